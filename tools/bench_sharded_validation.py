"""Times one validation pass of train.py of each kind, without and with --shard-validation, on one device (a world of
one: what is measured is the loss of the per-batch read-backs, not the split over ranks, which one GPU cannot show).

    python tools/bench_sharded_validation.py [--reps 15] [--out profiles/sharded_validation_bench.json]

  with_gt   train.validate_with_gt with DispResNet(18) on a generated set of 48 samples at 128 x 416 in batches of 4,
            ground truth of 128 x 416, images and ground truth already on the device
  losses    train.validate_without_gt with DispResNet(18) and PoseResNet(18) on the same images as 3-frame sequences
Each pass is timed with the host clock between device synchronisations, after a warm-up of both variants, the two
variants alternating in one process; per kind and variant the median, the minimum and the maximum of the repetitions
and every run are written, with the two variants' results.  Each run is a forward pass of its own through the
networks, whose outputs are not bit-reproducible from run to run, so the variants' results are compared at
1e-5 relative here, next to the spread of the host variant's own results over its repetitions (the exact comparisons,
on fixed inputs, are tests/test_gpu_sharded_validation.py's).  Writes one JSON file.  Needs a HIP device."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sc-sfmlearner-release_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

SAMPLES, B, H, W = 48, 4, 128, 416


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sharded_validation_bench.json"))
    cli = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_sharded_validation.py needs a HIP device")
    import models
    import train as T
    dev = torch.device("cuda", 0)
    T.device = dev
    torch.manual_seed(0)
    disp_net = models.DispResNet(18, False).to(dev)
    pose_net = models.PoseResNet(18, False).to(dev)
    gen = torch.Generator().manual_seed(1)
    rng = np.random.default_rng(1)
    K = torch.tensor([[0.58 * W, 0, 0.5 * W], [0, 1.92 * H, 0.5 * H], [0, 0, 1]]).expand(B, 3, 3).contiguous().to(dev)
    with_gt, losses = [], []
    for _ in range(SAMPLES // B):
        img = ((torch.rand(B, 3, H, W, generator=gen) - 0.45) / 0.225).to(dev)
        gt = rng.uniform(0.05, 90.0, (B, H, W)).astype(np.float32)
        gt[rng.random(gt.shape) < 0.7] = 0
        with_gt.append((img, torch.from_numpy(gt).to(dev)))
        refs = [(img + 0.05 * torch.randn(B, 3, H, W, generator=gen).to(dev)) for _ in range(2)]
        losses.append((img, refs, K, torch.inverse(K)))
    logger = types.SimpleNamespace(valid_bar=types.SimpleNamespace(update=lambda i: None),
                                   valid_writer=types.SimpleNamespace(write=lambda s: None))

    def args(flag):  # (train.py's default --print-freq: progress lines, and with the table a read-back, at batches 0 and 10)
        return types.SimpleNamespace(dataset="kitti", print_freq=10, shard_validation=flag, num_scales=1, with_ssim=1,
                                     with_mask=1, padding_mode="zeros")

    kinds = {"with_gt": lambda flag: T.validate_with_gt(args(flag), with_gt, disp_net, 0, logger)[0],
             "losses": lambda flag: T.validate_without_gt(args(flag), losses, disp_net, pose_net, 0, logger)[0]}

    def timed(fn, flag):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn(flag)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    result = {"device": torch.cuda.get_device_name(0), "samples": SAMPLES, "batch": B, "size": [H, W], "reps": cli.reps,
              "world": 1}
    for kind, fn in kinds.items():
        for flag in (False, True):  # warm-up: MIOpen's solvers, the libraries, the allocator
            fn(flag)
        runs = {False: [], True: []}
        values = {False: [], True: []}
        for _ in range(cli.reps):
            for flag in (False, True):
                ms, out = timed(fn, flag)
                runs[flag].append(ms)
                values[flag].append(out)
        host, table = np.array(values[False]), np.array(values[True])  # [reps, columns]
        worst = float(np.max(np.abs(host - table) / np.abs(host)))
        own = float(np.max(np.abs(host - host[0]) / np.abs(host[0])))
        if not worst <= 1e-5:
            raise SystemExit(f"{kind}: the two variants differ by {worst:.3e} relative")

        def stats(v):
            return {"median_ms": float(np.median(v)), "min_ms": float(np.min(v)), "max_ms": float(np.max(v)),
                    "runs_ms": [float(x) for x in v]}
        result[kind] = {"rank0_host_average": stats(runs[False]), "shard_validation": stats(runs[True]),
                        "median_ratio_host_over_table": float(np.median(runs[False]) / np.median(runs[True])),
                        "values_host": [float(x) for x in host[-1]], "values_table": [float(x) for x in table[-1]],
                        "worst_relative_difference_of_the_variants": worst,
                        "worst_relative_difference_of_the_host_variant_to_its_first_run": own}
    os.makedirs(os.path.dirname(os.path.abspath(cli.out)), exist_ok=True)
    with open(cli.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
