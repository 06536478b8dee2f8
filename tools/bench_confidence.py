"""Times the depth-consistency weights of scsfm_hip.confidence (libscsfm_conf.so; reconstruct.py --consistency-weight)
against the same arithmetic in torch operations on the device -- grid_sample and elementwise, what a user would otherwise
write -- and the weighted integration against the unweighted one.

    python tools/bench_confidence.py [--reps 15] [--out profiles/confidence_bench.json] [--dims 512 128 512] [--frames 64]

tools/bench_fusion.py's "drive" scene: 64 generated frames of 256 x 832 with their images and a 512 x 128 x 512 volume
(671 MB), all on the device.  Measured, alternating in one process after a warm-up of every variant:

  weights    all frames in one call at radius 1 and 2 (the pair records included), and the torch restatement of each; a
             sample is the time between two events round the call, the device idle before the first.  Reported per
             variant: median, minimum and maximum of --reps (at least 15) samples, the time per frame, and the bytes that
             must move (a frame's depth read once, its weight written once: 8 bytes a pixel; the taps come from L2) over
             the median.
  integrate  Volume.integrate of all frames into an emptied volume at 8 frames a launch, without and with weight=.

The results are compared first: the torch restatement agrees with the library to rounding, and a weight of all ones fuses
to the bits of the unweighted call.  Writes one JSON file.  Needs a HIP device."""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sc-sfmlearner-release_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

from bench_fusion import HBM_BYTES_PER_S, scene, stats  # noqa: E402

RADII = (1, 2)
FRAMES_PER_LAUNCH = 8


def torch_weights(disp, pair, max_depth):
    """include/scsfm_conf.h's weights (mean, min_views 1, floor 0) in torch operations, one slot after another over all
    the frames that have that neighbour"""
    depth = 1.0 / disp[:, 0]
    n, H, W = depth.shape
    radius = pair.shape[1] // 2
    dev = depth.device
    px = torch.arange(W, device=dev, dtype=torch.float32)[None, None, :]
    py = torch.arange(H, device=dev, dtype=torch.float32)[None, :, None]
    own = (depth > 0) & (depth <= max_depth)
    count = torch.zeros_like(depth)
    total = torch.zeros_like(depth)
    for s, o in enumerate(list(range(-radius, 0)) + list(range(1, radius + 1))):
        i0, i1 = max(0, -o), min(n, n - o)
        if i1 <= i0:
            continue
        c = pair[i0:i1, s].T[:, :, None, None]      # [16, m, 1, 1]
        d = depth[i0:i1]
        X, Y = (px - c[14]) / c[12] * d, (py - c[15]) / c[13] * d
        qx = c[0] * X + c[1] * Y + c[2] * d + c[9]
        qy = c[3] * X + c[4] * Y + c[5] * d + c[10]
        qz = c[6] * X + c[7] * Y + c[8] * d + c[11]
        u, v = c[12] * qx / qz + c[14], c[13] * qy / qz + c[15]
        g, h = torch.floor(u), torch.floor(v)
        ok = own[i0:i1] & (qz > 0) & (g >= 0) & (g <= W - 2) & (h >= 0) & (h <= H - 2)
        u, v = torch.where(ok, u, -2.0), torch.where(ok, v, -2.0)      # (no NaN reaches the sampler)
        grid = torch.stack([2 * u / (W - 1) - 1, 2 * v / (H - 1) - 1], dim=-1)
        nb = depth[i0 + o:i1 + o, None]
        p = torch.nn.functional.grid_sample(nb, grid, mode="bilinear", padding_mode="zeros", align_corners=True)[:, 0]
        low = -torch.nn.functional.max_pool2d(-nb, 2, 1)      # the smallest of a cell's four taps, [m, 1, H - 1, W - 1]
        cell = (torch.where(ok, h, 0).long() * (W - 1) + torch.where(ok, g, 0).long()).reshape(len(d), -1)
        ok &= (low.reshape(len(d), -1).gather(1, cell).reshape(d.shape) > 0)
        m = 1 - (qz - p).abs() / (qz + p)
        count[i0:i1] += ok
        total[i0:i1] += torch.where(ok, m, torch.zeros_like(m))
    mean = total / count.clamp(min=1)
    return torch.where((count > 0) & (mean >= 0), mean, torch.zeros_like(total))      # (a NaN becomes 0)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--dims", type=int, nargs=3, default=[512, 128, 512])
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--size", type=int, nargs=2, default=[256, 832])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "confidence_bench.json"))
    args = ap.parse_args(argv)
    if args.reps < 15:
        raise SystemExit("--reps: at least 15")
    if not torch.cuda.is_available():
        raise SystemExit("bench_confidence.py needs a HIP device")
    from scsfm_hip import _lib, confidence, fusion
    _lib.get_conf(), _lib.get_fuse()  # (a missing library is an error before anything is timed)
    dev = torch.device("cuda")
    F, (H, W), dims = args.frames, args.size, tuple(args.dims)
    voxel = 16.0 / max(dims)
    origin = (-0.5 * dims[0] * voxel + 0.6, -0.5 * dims[1] * voxel, -1.0)
    nvox = dims[0] * dims[1] * dims[2]
    disp, images, c2w, K, max_depth = scene(F, H, W, dev, "drive")

    def timed(fn):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    def run_hip(radius):
        return confidence.weights(disp, c2w, K, radius=radius, is_disp=True, max_depth=max_depth)

    def run_torch(radius):
        return torch_weights(disp, confidence.pair_cameras(c2w, K, radius), max_depth)

    # results first (this is the warm-up of every variant too)
    agree, mean = {}, {}
    for r in RADII:
        got, want = run_hip(r), run_torch(r)
        agree[r] = float(((got - want).abs() <= 1e-4).float().mean())
        mean[r] = float(got.double().mean())
        print(f"radius {r}: {F} frames of {H} x {W}; mean weight {mean[r]:.6f}, {float((got == 0).float().mean()):.4f} at zero; "
              f"torch agrees on {100 * agree[r]:.3f} % of the pixels", flush=True)
    weight = run_hip(1)
    vols = {k: fusion.Volume(dims, origin, voxel, device=dev, frames_per_launch=FRAMES_PER_LAUNCH) for k in ("plain", "weighted")}

    def run_plain():
        vols["plain"].integrate(disp, images, c2w, K, is_disp=True, max_depth=max_depth)

    def run_weighted(w=weight):
        vols["weighted"].integrate(disp, images, c2w, K, is_disp=True, max_depth=max_depth, weight=w)

    run_plain()
    run_weighted(torch.ones_like(weight))
    ones_same = bool(torch.equal(vols["plain"].planes.view(torch.int32), vols["weighted"].planes.view(torch.int32)))
    vols["weighted"].planes.zero_()
    run_weighted()
    print(f"volume {dims}, {20 * nvox / 1e6:.0f} MB; a weight of ones fuses to the unweighted bits: {ones_same}", flush=True)

    t_hip, t_torch = {r: [] for r in RADII}, {r: [] for r in RADII}
    t_plain, t_weighted = [], []
    for _ in range(args.reps):
        for r in RADII:
            t_hip[r].append(timed(lambda: run_hip(r)))
            t_torch[r].append(timed(lambda: run_torch(r)))
        vols["plain"].planes.zero_()
        t_plain.append(timed(run_plain))
        vols["weighted"].planes.zero_()
        t_weighted.append(timed(run_weighted))

    entries = []
    for r in RADII:
        e = {"radius": r, "hip": stats(t_hip[r]), "torch": stats(t_torch[r]), "torch_agrees_share": agree[r],
             "mean_weight": mean[r]}
        e["hip"]["ms_per_frame"] = e["hip"]["median_ms"] / F
        e["hip"]["bytes"] = 8 * F * H * W
        e["hip"]["bytes_per_s"] = e["hip"]["bytes"] / (e["hip"]["median_ms"] * 1e-3)
        e["hip"]["share_of_hbm_rate"] = e["hip"]["bytes_per_s"] / HBM_BYTES_PER_S
        e["ratio_torch_over_hip"] = e["torch"]["median_ms"] / e["hip"]["median_ms"]
        entries.append(e)
        print(f"weights, radius {r}: {e['hip']['median_ms']:.3f} ms ({e['hip']['min_ms']:.3f} .. {e['hip']['max_ms']:.3f}), "
              f"{e['hip']['bytes_per_s'] / 1e12:.3f} TB/s; torch {e['torch']['median_ms']:.2f} ms "
              f"({e['torch']['min_ms']:.2f} .. {e['torch']['max_ms']:.2f}): {e['ratio_torch_over_hip']:.0f} times", flush=True)
    integ = {"frames_per_launch": FRAMES_PER_LAUNCH, "plain": stats(t_plain), "weighted": stats(t_weighted),
             "ones_leave_the_unweighted_bits": ones_same}
    for k in ("plain", "weighted"):
        integ[k]["ms_per_frame"] = integ[k]["median_ms"] / F
    integ["ratio_weighted_over_plain"] = integ["weighted"]["median_ms"] / integ["plain"]["median_ms"]
    print(f"integrate, {FRAMES_PER_LAUNCH} frames a launch: {integ['plain']['median_ms']:.2f} ms "
          f"({integ['plain']['min_ms']:.2f} .. {integ['plain']['max_ms']:.2f}) unweighted, {integ['weighted']['median_ms']:.2f} ms "
          f"({integ['weighted']['min_ms']:.2f} .. {integ['weighted']['max_ms']:.2f}) weighted", flush=True)
    result = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "dims": list(dims), "voxels": nvox, "frames": F,
              "frame_size": [H, W], "scene": "drive", "max_depth": max_depth, "hbm_bytes_per_s": HBM_BYTES_PER_S,
              "weights": entries, "integrate": integ}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps({k: v for k, v in result.items() if k not in ("weights", "integrate")}))


if __name__ == "__main__":
    main()
