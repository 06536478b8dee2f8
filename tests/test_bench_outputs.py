"""bench.py's --dump-outputs and the result line's headline fields, without a GPU: the writer keeps float64 where the
value is float64 and float32 otherwise and refuses a set above its limit, the sample of a flattened set is fixed by its seed,
and `value` / `ms_per_step` are the K timed steps' rate and time per step."""
import argparse
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def test_write_outputs_dtypes_names_and_limit(tmp_path):
    import bench
    arrays = {"loss": torch.tensor(1.25, dtype=torch.float64), "grad": torch.arange(6, dtype=torch.float16).reshape(2, 3),
              "count": 3}
    n = bench.write_outputs(str(tmp_path / "out"), arrays)
    got = {p.name: np.load(p) for p in (tmp_path / "out").iterdir()}
    assert set(got) == {"loss.npy", "grad.npy", "count.npy"} and n == sum(a.nbytes for a in got.values())
    assert got["loss.npy"].dtype == np.float64 and float(got["loss.npy"]) == 1.25
    assert got["grad.npy"].dtype == np.float32 and got["grad.npy"].shape == (2, 3) and got["grad.npy"][1, 2] == 5
    assert got["count.npy"].dtype == np.float32
    with pytest.raises(ValueError):
        bench.write_outputs(str(tmp_path / "big"), {"x": torch.zeros(1000)}, limit_bytes=3999)
    assert not (tmp_path / "big").exists()  # nothing written when the set is refused


def test_flat_sample_is_fixed_by_its_seed():
    import bench
    net = torch.nn.Sequential(torch.nn.Linear(50, 40), torch.nn.Linear(40, 30))
    ts = list(net.parameters())
    n = sum(p.numel() for p in ts)
    a, b = bench.flat_sample(ts, k=500), bench.flat_sample(ts, k=500)
    assert a.dtype == torch.float32 and a.numel() == 500 and torch.equal(a, b)
    assert not torch.equal(a, bench.flat_sample(ts, k=500, seed=1))
    flat = torch.cat([p.detach().reshape(-1) for p in ts])
    assert torch.equal(bench.flat_sample(ts, k=n + 1), flat)  # fewer entries than the sample: all of them, in order
    assert all(bool((flat == v).any()) for v in a[:20])


def test_headline_value_and_ms_per_step_are_those_of_the_timed_steps():
    import bench
    args = argparse.Namespace(dataset="kitti", height=256, width=832, batch=12, n_ref=2, resnet_layers=18, steps=20, warmup=5,
                              exact=0, channels_last=0)
    e2e = {"elapsed_s": 2.0, "ranks": 1, "final_loss": 2.5, "model": "m", "trainable_parameters": 26828186}
    r = bench.headline(args, 1, None, False, e2e)
    assert r["metric"] == "train images/sec (+ warp-loss ms/step) KITTI 256x832 RN18"
    assert r["value"] == 120.0 and r["ms_per_step"] == 100.0 and r["unit"] == "images/s" and r["higher_is_better"] is True
    assert r["dtype"] == "f32" and r["steps"] == 20 and r["warmup"] == 5 and r["rccl_ranks"] == 1
    assert r["train"]["final_loss"] == 2.5 and r["config"]["parallelism"] == "1 GPU"
    hot = bench.headline(args, 1, None, False, None, hot_rate=1000.0, loss_ms=0.5)
    assert hot["value"] == 1000.0 and hot["ms_per_step"] == 0.5 and "hot path ONLY" in hot["metric"] and hot["train"] is None


def test_full_and_dump_outputs_are_options():
    import subprocess
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "--full" in out.stdout and "--dump-outputs DIR" in out.stdout
