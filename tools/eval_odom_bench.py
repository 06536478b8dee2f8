"""Times the odometry path on the GPU against the host (record, not a gate) -> profiles/odom_eval_bench.json

    python tools/eval_odom_bench.py [--out profiles/odom_eval_bench.json] [--skip-vo]

 (a) evaluate_odometry over the eleven KITTI sequence lengths (synthetic poses), inputs on the device, against the
     oracle's numpy evaluation of the same input on the host;
 (b) chain_poses for 4,661 pose vectors against the sequential host fold;
 (c) test_vo.py's network loop: image pairs per second at batch 1 and batch 8 (random weights, synthetic frames).
Warm-up first, then alternating repetitions; medians and minima are recorded.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "sc-sfmlearner-release_amd")]

import odom_eval_oracle as O  # noqa: E402
from scsfm_hip import odometry  # noqa: E402

KITTI_LENGTHS = (4541, 1101, 4661, 801, 271, 2761, 1101, 1101, 4071, 1591, 1201)


def trajectories(seed=0):
    rng = np.random.default_rng(seed)
    gts, preds = [], []
    for n in KITTI_LENGTHS:
        vec = np.zeros((n - 1, 6))
        vec[:, 2] = -rng.uniform(0.6, 1.2)
        vec[:, 4] = 0.003 * np.sin(np.arange(n - 1) / rng.uniform(20, 60))
        noisy = vec * np.array([0.04] * 3 + [1.0] * 3) + rng.normal(0, 2e-4, vec.shape)
        gts.append(O.fold(O.euler_mat(vec)).reshape(-1, 12))
        preds.append(O.fold(O.euler_mat(noisy)).reshape(-1, 12))
    return gts, preds


def timed(fn, reps, sync=True):
    out = []
    for _ in range(reps):
        if sync:
            torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        if sync:
            torch.cuda.synchronize()
        out.append((time.perf_counter() - t) * 1e3)
    return out


def stats(ms):
    return dict(median_ms=statistics.median(ms), min_ms=min(ms), reps=len(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "odom_eval_bench.json"))
    ap.add_argument("--skip-vo", action="store_true")
    args = ap.parse_args()
    rec = dict(device=torch.cuda.get_device_name(0), kitti_lengths=KITTI_LENGTHS)

    gts, preds = trajectories()
    d_gts, d_preds = [torch.from_numpy(g).cuda() for g in gts], [torch.from_numpy(p).cuda() for p in preds]
    for alignment in (None, "7dof"):
        gpu = lambda: odometry.evaluate_odometry(d_gts, d_preds, alignment)
        host = lambda: O.evaluate(gts, preds, alignment)
        timed(gpu, 5)
        g, h = [], []
        for _ in range(3):  # alternating
            g += timed(gpu, 10)
            h += timed(host, 1, sync=False)
        rec[f"evaluate_{alignment or 'none'}"] = dict(gpu=stats(g), host_numpy=stats(h), launches_per_call=5,
                                                      frames=int(sum(KITTI_LENGTHS)))

    vec = torch.from_numpy(np.random.default_rng(1).normal(0, 0.01, (4661, 6)).astype(np.float32)).cuda()
    gpu = lambda: odometry.chain_poses(vec)
    mats = O.euler_mat(vec.cpu().numpy())

    def host():
        g = np.eye(4)
        for m in mats:  # test_vo.py's loop
            g = g @ np.linalg.inv(np.vstack([m, [0, 0, 0, 1]]))

    timed(gpu, 5)
    g, h = [], []
    for _ in range(3):
        g += timed(gpu, 20)
        h += timed(host, 1, sync=False)
    rec["chain_4661"] = dict(gpu=stats(g), host_fold=stats(h), launches_per_call=3)

    if not args.skip_vo:
        import models
        net = models.PoseResNet(18, False).cuda().eval()
        frames = torch.randn(33, 3, 256, 832, device="cuda")
        with torch.no_grad():
            for bs in (1, 8):
                def run():
                    for j in range(0, 32, bs):
                        net(frames[j:j + bs], frames[j + 1:j + 1 + bs])
                timed(run, 2)
                ms = timed(run, 5)
                rec[f"test_vo_pairs_per_s_batch{bs}"] = 32 / (statistics.median(ms) * 1e-3)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
