"""Times the metric step of train.py --with-gt's validation (no dataset and no network needed): from the network's
disparity [4, 1, 256, 832] and a KITTI-like ground truth [4, 375, 1242] on the device to the six Python floats.

    python tools/bench_validation_errors.py [--reps 15] [--batches 200] [--out profiles/validation_errors_bench.json]

  library   scsfm_hip.validation.depth_errors(..., is_disp=True) + batch_mean: one call of libscsfm_val.so, one read-back
  torch     the sequence it replaces: 1 / disp, F.interpolate to the ground truth's size, compute_errors' torch body
            (selected with scsfm_hip.config.set_errors_on_torch, in the same process)
Both are timed with the host clock between device synchronisations (both end in a read-back; the torch body also
synchronises twice per image), after a warm-up of each, alternating, first for one batch (median, minimum and maximum
of the repetitions) and then for an epoch of --batches batches cycling over eight different ones (median of three).
The two paths' results on every batch are compared at rtol 1e-5.  Writes one JSON file.  Needs a HIP device."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sc-sfmlearner-release_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

B, H, W = 4, 375, 1242
h, w = 256, 832
DISTINCT = 8


def make_batch(rng, dev):
    """A disparity like DispResNet's (sigmoid-scaled, nearer towards the bottom rows) and a ground truth like KITTI's
    projected lidar: multiples of 1/256, about 70 % zeros, nothing in the top third."""
    ramp = np.linspace(0.02, 0.6, h, dtype=np.float32)[None, :, None]
    disp = (ramp * rng.uniform(0.7, 1.4, (B, h, w))).astype(np.float32) + np.float32(0.01)
    depth = (1 / np.linspace(0.012, 0.5, H, dtype=np.float32))[None, :, None] * rng.uniform(0.6, 1.6, (B, H, W))
    gt = (np.round(depth * 256) / 256).astype(np.float32)
    gt[rng.random((B, H, W)) < 0.7] = 0
    gt[:, :H // 3] = 0
    return torch.from_numpy(gt).to(dev), torch.from_numpy(disp[:, None]).to(dev)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--batches", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "validation_errors_bench.json"))
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_validation_errors.py needs a HIP device")
    import loss_functions as LF
    from scsfm_hip import config, validation
    dev = torch.device("cuda")
    rng = np.random.default_rng(0)
    batches = [make_batch(rng, dev) for _ in range(DISTINCT)]

    def library(gt, disp):
        return validation.batch_mean(validation.depth_errors(gt, disp, "kitti", is_disp=True))

    @torch.no_grad()
    def torch_path(gt, disp):
        depth = 1 / disp[:, 0]
        depth = F.interpolate(depth.unsqueeze(1), [H, W]).squeeze(1)
        config.set_errors_on_torch(True)
        try:
            return LF.compute_errors(gt, depth, "kitti")
        finally:
            config.set_errors_on_torch(False)

    def timed(fn, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for k in range(n):
            fn(*batches[k % DISTINCT])
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    worst = 0.0
    for gt, disp in batches:  # (also the warm-up of every shape of both paths)
        a, b = np.array(library(gt, disp)), np.array(torch_path(gt, disp))
        worst = max(worst, float(np.max(np.abs(a - b) / np.abs(b))))
    valid = int(validation.depth_errors(*batches[0], "kitti", is_disp=True).count.sum())

    one = {"library": [], "torch": []}
    for _ in range(args.reps):
        one["library"].append(timed(library, 1))
        one["torch"].append(timed(torch_path, 1))
    epoch = {"library": [], "torch": []}
    for _ in range(3):
        epoch["library"].append(timed(library, args.batches))
        epoch["torch"].append(timed(torch_path, args.batches))

    def stats(v):
        return {"median_ms": float(np.median(v)), "min_ms": float(np.min(v)), "max_ms": float(np.max(v)),
                "runs_ms": [float(x) for x in v]}

    result = {"device": torch.cuda.get_device_name(0), "batch": B, "pred": [h, w], "gt": [H, W], "dataset": "kitti",
              "valid_pixels_first_batch": valid, "reps": args.reps, "epoch_batches": args.batches,
              "one_batch": {k: stats(v) for k, v in one.items()},
              "epoch": {k: stats(v) for k, v in epoch.items()},
              "one_batch_ratio_torch_over_library": float(np.median(one["torch"]) / np.median(one["library"])),
              "epoch_ratio_torch_over_library": float(np.median(epoch["torch"]) / np.median(epoch["library"])),
              "worst_relative_difference_of_the_six_metrics": worst}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))
    if not worst <= 1e-5:
        raise SystemExit(f"the two paths differ by {worst:.3e} relative")


if __name__ == "__main__":
    main()
