"""scsfm_hip/training_state.py and the command line around it: a state goes through a file and comes back field for
field; the write is atomic; the logs are cut to the recorded rows; train.py refuses, at argument parsing and without a
device, what it cannot continue; a state written by torch.optim.Adam loads into scsfm_hip.optim.Adam and back with every
moment's bits (the one-launch Adam on tests/hostsim, swapped in from outside)."""
import argparse
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

from scsfm_hip import training_state as TS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRAIN = os.path.join(ROOT, "sc-sfmlearner-release_amd", "train.py")
ARGS = dict(resnet_layers=18, sequence_length=3, num_scales=1, optimizer="torch", freeze_bn="off", seed=0, batch_size=2)


def _args(save_path, **kw):
    return argparse.Namespace(save_path=str(save_path), log_summary="progress_log_summary.csv",
                              log_full="progress_log_full.csv", **{**ARGS, **kw})


def _logs(args, summary, full):
    for name, rows in ((args.log_summary, summary), (args.log_full, full)):
        with open(os.path.join(args.save_path, name), "w") as f:
            f.write("header\n" + "".join("row {}\n".format(i) for i in range(rows)))


def _optimizer(cls=torch.optim.Adam, steps=2):
    g = torch.Generator().manual_seed(3)
    params = [torch.nn.Parameter(torch.randn(s, generator=g)) for s in ((5, 3), (2049,), (7,))]
    opt = cls([{"params": params[:2], "lr": 1e-3}, {"params": params[2:], "lr": 1e-2}], betas=(0.9, 0.999),
              weight_decay=0.01)
    for _ in range(steps):
        for p in params[:2]:  # (the last one never has a gradient: it has no state)
            p.grad = torch.randn(p.shape, generator=g)
        opt.step()
    return params, opt


def test_capture_and_restore_round_trip_every_field_through_a_file(tmp_path):
    args = _args(tmp_path)
    _logs(args, 3, 12)
    params, opt = _optimizer()
    random.seed(11)
    np.random.seed(12)
    torch.manual_seed(13)
    state = TS.capture(args, 3, 17, 0.125, opt, torch.device("cpu"))
    drawn = (random.random(), np.random.rand(), torch.rand(3))
    path = TS.save(state, args.save_path)
    assert path == os.path.join(str(tmp_path), TS.STATE_FILE) and os.listdir(tmp_path).count(TS.STATE_FILE) == 1
    assert not [n for n in os.listdir(tmp_path) if n.endswith(".tmp")]
    for source in (str(tmp_path), path):  # a run directory or its state file
        assert TS.locate(source) == (str(tmp_path), path)
    back = TS.load(str(tmp_path))
    assert set(back) == {"version", "epoch", "n_iter", "best_error", "optimizer", "log_rows", "rng", "args"}
    assert (back["version"], back["epoch"], back["n_iter"], back["best_error"]) == (1, 3, 17, 0.125)
    assert back["log_rows"] == {"summary": 3, "full": 12} and back["args"] == ARGS
    assert set(back["rng"]) == {"python", "numpy", "torch", "device"} and back["rng"]["device"] is None
    # an epoch that was cut short left rows behind; the generators have moved on
    _logs(args, 3, 14)
    _, fresh = _optimizer(steps=0)
    assert TS.restore(back, args, fresh, torch.device("cpu")) == (3, 17, 0.125)
    again = (random.random(), np.random.rand(), torch.rand(3))
    assert again[0] == drawn[0] and again[1] == drawn[1] and torch.equal(again[2], drawn[2])
    assert TS.log_rows(os.path.join(args.save_path, args.log_full)) == 12
    assert open(os.path.join(args.save_path, args.log_full)).read().endswith("row 11\n")
    a, b = opt.state_dict(), fresh.state_dict()
    assert sorted(a["state"]) == sorted(b["state"]) == [0, 1] and a["param_groups"] == b["param_groups"]
    for i in a["state"]:
        assert all(torch.equal(a["state"][i][k], b["state"][i][k]) for k in ("step", "exp_avg", "exp_avg_sq"))


def test_restore_without_generators_and_on_another_rank(tmp_path):
    args = _args(tmp_path)
    _logs(args, 1, 2)
    _, opt = _optimizer()
    torch.manual_seed(13)
    state = TS.capture(args, 1, 1, 0.5, opt, None)
    drawn = torch.rand(3)
    torch.manual_seed(99)
    TS.restore(state, args, opt, None, generators=False)
    assert not torch.equal(torch.rand(3), drawn)
    os.remove(os.path.join(args.save_path, args.log_full))  # ranks other than 0 do not touch the logs
    TS.restore(state, args, opt, None, rank=1, world=2)
    r1 = torch.rand(3)
    TS.restore(state, args, opt, None, rank=2, world=3)
    assert not torch.equal(r1, drawn) and not torch.equal(torch.rand(3), r1)
    TS.restore(state, args, opt, None, rank=1, world=2)
    assert torch.equal(torch.rand(3), r1)  # (from the seed, the epoch and the rank: the same every time)


def test_a_failing_write_leaves_the_old_file(tmp_path, monkeypatch):
    args = _args(tmp_path)
    _logs(args, 1, 2)
    _, opt = _optimizer()
    path = TS.save(TS.capture(args, 1, 1, 0.5, opt, None), args.save_path)
    before = open(path, "rb").read()

    def dies(obj, f, *a, **k):
        with open(f, "wb") as out:
            out.write(b"half a file")
        raise OSError("killed")
    monkeypatch.setattr(torch, "save", dies)
    with pytest.raises(OSError, match="killed"):
        TS.save(TS.capture(args, 2, 2, 0.25, opt, None), args.save_path)
    monkeypatch.undo()
    assert open(path, "rb").read() == before and TS.load(path)["epoch"] == 1
    assert sorted(os.listdir(tmp_path)) == sorted([TS.STATE_FILE, args.log_summary, args.log_full])


def test_logs_are_cut_to_the_recorded_rows(tmp_path):
    log = tmp_path / "log.csv"
    log.write_text("a\tb\n1\t2\n3\t4\n5\t6\n")
    assert TS.log_rows(str(log)) == 3
    TS.truncate_log(str(log), 2)
    assert log.read_text() == "a\tb\n1\t2\n3\t4\n"
    TS.truncate_log(str(log), 2)
    assert log.read_text() == "a\tb\n1\t2\n3\t4\n"
    TS.truncate_log(str(log), 0)
    assert log.read_text() == "a\tb\n" and TS.log_rows(str(log)) == 0
    with pytest.raises(ValueError, match="data rows"):
        TS.truncate_log(str(log), 1)  # (a log shorter than the state says is another run's)


@pytest.fixture(scope="module")
def run_dir(tmp_path_factory):
    """a run directory as --save-state leaves it after one epoch (the checkpoints only have to be there)"""
    d = tmp_path_factory.mktemp("run")
    args = _args(d)
    _logs(args, 1, 2)
    _, opt = _optimizer()
    TS.save(TS.capture(args, 1, 1, 0.5, opt, None), args.save_path)
    for name in TS.CHECKPOINTS:
        torch.save({"epoch": 1, "state_dict": {}}, os.path.join(str(d), name))
    return d


def _train(*argv):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="")
    r = subprocess.run([sys.executable, TRAIN, "synthetic:8:64x96", "--name", "t", "--with-pretrain", "0", "-b", "2",
                        "-j", "0", *argv], capture_output=True, text=True, env=env, timeout=120)
    return r.returncode, r.stderr


@pytest.mark.parametrize("extra, message", [
    (["--pretrained-disp", "x.pth.tar"], "cannot be combined with --pretrained-disp / --pretrained-pose"),
    (["--pretrained-pose", "x.pth.tar"], "cannot be combined with --pretrained-disp / --pretrained-pose"),
    (["--resnet-layers", "50"], "resnet_layers 18, this command line says 50"),
    (["--sequence-length", "5"], "sequence_length 3, this command line says 5"),
    (["--num-scales", "4"], "num_scales 1, this command line says 4"),
    (["--optimizer", "hip"], "optimizer torch, this command line says hip"),
    (["--freeze-bn", "stats"], "freeze_bn off, this command line says stats"),
    (["--seed", "1"], "seed 0, this command line says 1"),
    (["-b", "4"], "batch_size 2, this command line says 4"),
    (["--epochs", "1"], "has completed 1 epochs, --epochs 1 leaves nothing to do"),
])
def test_train_py_refuses_at_argument_parsing(run_dir, extra, message):
    code, err = _train("--resume", str(run_dir), "--epochs", "3", *extra)
    assert code == 2 and message in err, err


def test_train_py_refuses_a_path_without_a_state_or_a_checkpoint(run_dir, tmp_path):
    code, err = _train("--resume", str(tmp_path))
    assert code == 2 and "there is no state file" in err, err
    code, err = _train("--resume", str(tmp_path / "nowhere" / TS.STATE_FILE))
    assert code == 2 and "there is no state file" in err, err
    for missing in TS.CHECKPOINTS:
        for name in os.listdir(run_dir):
            if name != missing:
                os.link(os.path.join(run_dir, name), tmp_path / name) if not (tmp_path / name).exists() else None
        code, err = _train("--resume", str(tmp_path))
        assert code == 2 and "lacks " + missing in err, err
        for name in os.listdir(tmp_path):
            os.remove(tmp_path / name)


def test_refusals_are_those_of_the_function(run_dir):
    """(what the subprocesses above print is ``refusal``'s; an acceptable command line passes it)"""
    ok = argparse.Namespace(resume=str(run_dir), pretrained_disp=None, pretrained_pose=None, epochs=2, **ARGS)
    assert TS.refusal(ok) is None
    ok.resume = os.path.join(str(run_dir), TS.STATE_FILE)
    assert TS.refusal(ok) is None


def test_freeze_bn_takes_resume_as_a_source_of_weights(run_dir):
    import train as T
    args = T.parser.parse_args(["d", "--name", "t", "--with-pretrain", "0", "--freeze-bn", "stats"])
    assert len(T.nets_without_statistics(args)) == 2
    args.resume = str(run_dir)
    assert T.nets_without_statistics(args) == []


def test_a_torch_state_loads_into_the_hip_optimiser_and_back(tmp_path, monkeypatch):
    import _hostsim_opt
    from scsfm_hip import _lib, optim
    monkeypatch.setattr(_lib, "get_opt", _hostsim_opt.lib)
    monkeypatch.setattr(optim, "_need_cuda", lambda *a: None)
    _, theirs = _optimizer(torch.optim.Adam)
    torch.save(theirs.state_dict(), tmp_path / "torch.pth")
    params, ours = _optimizer(optim.Adam, steps=0)
    ours.load_state_dict(torch.load(tmp_path / "torch.pth", weights_only=False))
    a, b = theirs.state_dict(), ours.state_dict()
    assert sorted(b["state"]) == [0, 1] and b["param_groups"] == a["param_groups"]
    assert list(ours._steps) == [2, 2, 0]
    for i in a["state"]:
        assert b["state"][i]["exp_avg"].shape == a["state"][i]["exp_avg"].shape
        assert all(torch.equal(a["state"][i][k].view(torch.int32) if k != "step" else a["state"][i][k],
                               b["state"][i][k].view(torch.int32) if k != "step" else b["state"][i][k])
                   for k in ("step", "exp_avg", "exp_avg_sq"))
    # a step under ours: the first two advance to 3, the third is still without state; then back into torch's
    g = torch.Generator().manual_seed(8)
    for p in params[:2]:
        p.grad = torch.randn(p.shape, generator=g)
    ours.step()
    torch.save(ours.state_dict(), tmp_path / "hip.pth")
    _, back = _optimizer(torch.optim.Adam, steps=0)
    back.load_state_dict(torch.load(tmp_path / "hip.pth", weights_only=False))
    c, d = ours.state_dict(), back.state_dict()
    assert sorted(d["state"]) == [0, 1] and all(float(d["state"][i]["step"]) == 3.0 for i in (0, 1))
    for i in c["state"]:
        assert all(torch.equal(c["state"][i][k].view(torch.int32), d["state"][i][k].view(torch.int32))
                   for k in ("exp_avg", "exp_avg_sq"))
    for p in list(back.param_groups[0]["params"]):
        p.grad = torch.ones_like(p)
    back.step()  # (torch accepts the state it was given)
    assert float(back.state_dict()["state"][0]["step"]) == 4.0


def test_the_hip_optimiser_refuses_what_it_does_not_do(monkeypatch):
    from scsfm_hip import optim
    p = torch.nn.Parameter(torch.ones(4))
    with pytest.raises(RuntimeError, match="HIP device"):
        optim.Adam([p])
    monkeypatch.setattr(optim, "_need_cuda", lambda *a: None)
    for kw in (dict(amsgrad=True), dict(maximize=True), dict(capturable=True), dict(differentiable=True),
               dict(betas=(1.0, 0.999)), dict(eps=float("inf"))):
        with pytest.raises(ValueError):
            optim.Adam([p], **kw)
    for bad in (torch.ones(4, dtype=torch.float64), torch.ones(4, 4).t()):
        with pytest.raises(ValueError, match="contiguous fp32"):
            optim.Adam([torch.nn.Parameter(bad)])
    q = torch.nn.Parameter(torch.ones(4, 4))
    opt = optim.Adam([q])
    q.grad = torch.ones(4, 4).t()  # (not contiguous)
    with pytest.raises(RuntimeError, match="contiguous fp32 gradients"):
        opt.step()
    with pytest.raises(RuntimeError, match="cannot be added"):
        opt.add_param_group({"params": [torch.nn.Parameter(torch.ones(2))]})
