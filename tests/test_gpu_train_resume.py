"""train.py --save-state / --resume as subprocesses on the device, at tests/test_gpu_trainer.py's shapes: one epoch of two
steps with --save-state, then --resume of that directory up to two epochs, once per optimiser; and a state saved under
one optimiser is refused under the other.

The loss path's float atomics and MIOpen's solver choice make two GPU runs differ in their last bits, so this test checks
the BOOKKEEPING of a resumed run -- one directory, the logs' rows, the checkpoints' epoch, the counters, the best error,
the step counts, which tensors have state.  That a resumed run is the straight run bit for bit is tests/test_resume_cpu.py's
claim, on the deterministic host path."""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "sc-sfmlearner-release_amd")
EPOCH_SIZE = 2


def _train(cwd, *argv):
    cmd = ["timeout", "-k", "10", "600", sys.executable, os.path.join(PKG, "train.py"), "synthetic:8:128x416",
           "--resnet-layers", "18", "--num-scales", "1", "-b", "2", "--epoch-size", str(EPOCH_SIZE), "--sequence-length", "3",
           "--with-auto-mask", "1", "--with-pretrain", "0", "-j", "0", "--name", "resume", *argv]
    env = dict(os.environ, PYTHONPATH=PKG, SCSFM_CUDNN_BENCHMARK="0")
    return subprocess.run(cmd, cwd=cwd, env=env, capture_output=True, text=True)


def _unused_heads():
    """the indices, in train.py's parameter order, of DispResNet's output convolutions of the scales the loss never reads"""
    sys.path.insert(0, PKG)
    import models
    disp, pose = models.DispResNet(18, False), models.PoseResNet(18, False)
    dec = disp.decoder
    unused = {id(p) for scale, idx in dec._head.items() if scale >= 1 for p in dec.decoder[idx].parameters()}
    params = [p for net in (disp, pose) for p in net.parameters() if p.requires_grad]  # (as train.py forms them)
    return {k for k, p in enumerate(params) if id(p) in unused}, len(params)


@pytest.mark.parametrize("optimizer", ["hip", "torch"])
def test_a_run_is_continued_in_its_directory(tmp_path, optimizer):
    out = _train(tmp_path, "--epochs", "1", "--save-state", "--optimizer", optimizer)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    runs = os.path.join(tmp_path, "checkpoints", "resume")
    (stamp,) = os.listdir(runs)
    run = os.path.join(runs, stamp)
    first = torch.load(os.path.join(run, "train_state.pth.tar"), map_location="cpu", weights_only=False)
    assert first["epoch"] == 1 and first["n_iter"] == EPOCH_SIZE - 1 and first["log_rows"] == {"summary": 1, "full": 2}
    assert first["args"]["optimizer"] == optimizer

    out = _train(tmp_path, "--epochs", "2", "--resume", run, "--optimizer", optimizer)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert "=> resuming {} at epoch 1 (n_iter {}, best_error {})".format(run, EPOCH_SIZE - 1, first["best_error"]) in out.stdout
    assert os.listdir(runs) == [stamp]  # still one run directory
    full = open(os.path.join(run, "progress_log_full.csv")).read().strip().split("\n")
    summary = open(os.path.join(run, "progress_log_summary.csv")).read().strip().split("\n")
    assert full[0].split("\t")[0] == "train_loss" and len(full) == 1 + 2 * EPOCH_SIZE
    assert summary[0].split("\t") == ["train_loss", "validation_loss"] and len(summary) == 1 + 2
    for name in ("dispnet_checkpoint.pth.tar", "exp_pose_checkpoint.pth.tar"):
        assert torch.load(os.path.join(run, name), map_location="cpu")["epoch"] == 2
    state = torch.load(os.path.join(run, "train_state.pth.tar"), map_location="cpu", weights_only=False)
    # (n_iter does not count an epoch's last step: train.py:296-298 of the reference breaks before the increment)
    assert state["epoch"] == 2 and state["n_iter"] == 2 * (EPOCH_SIZE - 1)
    assert state["log_rows"] == {"summary": 2, "full": 2 * EPOCH_SIZE}
    decisive = [float(row.split("\t")[1]) for row in summary[1:]]
    assert state["best_error"] == min(decisive) and first["best_error"] == decisive[0]
    unused, n_params = _unused_heads()
    steps = {i: float(s["step"]) for i, s in state["optimizer"]["state"].items()}
    assert len(unused) == 6 and set(steps) == set(range(n_params)) - unused  # the unused scale heads have no state
    assert set(steps.values()) == {2.0 * EPOCH_SIZE}
    assert not [n for n in os.listdir(run) if n.endswith(".tmp")]

    if optimizer == "torch":
        # the file formats interchange, a run's arithmetic does not change silently: refused at argument parsing
        out = _train(tmp_path, "--epochs", "3", "--resume", run, "--optimizer", "hip")
        assert out.returncode == 2 and "optimizer torch, this command line says hip" in out.stderr, out.stderr[-2000:]
        assert os.listdir(runs) == [stamp]
