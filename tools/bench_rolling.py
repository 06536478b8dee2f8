"""Times the moving volume of scsfm_hip.rolling (libscsfm_roll.so; reconstruct.py --follow): the shift against the same
move written as torch slice copies, the extraction of the points that leave against the extraction of the whole volume,
and --follow's loop along a generated drive against one dense volume that covers the whole path.

    python tools/bench_rolling.py [--reps 15] [--out profiles/rolling_bench.json] [--dims 512 128 512]

Medians of --reps (at least 15) samples, the variants alternating in one process after a warm-up of each; a sample is the
time between two events round the calls, the device idle before the first, allocations included.

  shift      RollingVolume.move by (0, 0, 8) and by (8, 0, 0) in the 512 x 128 x 512 volume of tools/bench_fusion.py, fused
             with its "drive" scene.  The yardstick is torch: a zeroed buffer of the same size and one slice copy into it.
             The algorithmic bytes are 2 x 20 bytes a voxel (every element read once and written once); they are given
             over the median as bytes per second and as a share of the 8 TB/s HBM rate.  The first move of each kind is
             compared with torch's, by bits.
  leaving    RollingVolume.leaving for those two shifts (count, one int to the host, extract) at min_weight 2.  The
             yardstick is Volume.extract of the whole volume, the only way to those points without the keep box.
  follow     256 frames of 256 x 832 on bench_fusion's "drive" law (20.4 units forward, 5.1 sideways, turning), voxels of
             1 / 32, depths to 2.5: a window of 184 voxels a side (5.75 units: the drive is three and a half to four
             windows long), placed before every batch of 8 frames as reconstruct.py --follow places it, the leaving points
             copied to the host, against the same frames into one dense volume over the whole path (the cameras' box grown
             by the depth limit) at the same voxel size.  Reported: the time, the peak of the device memory allocated on
             top of the frames, the number of shifts, the share of the time between the events round them, the points.

Writes one JSON file.  Needs a HIP device."""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sc-sfmlearner-release_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench_fusion import HBM_BYTES_PER_S, scene, stats  # noqa: E402

SHIFTS = ((0, 0, 8), (8, 0, 0))
FOLLOW = dict(frames=256, voxel=1.0 / 32, max_depth=2.5, step=8, batch=8, min_weight=2.0)


def timed(fn):
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def torch_shift(src, s):
    """the move in torch: a zeroed buffer and one slice copy"""
    out = torch.zeros_like(src)
    _, nz, ny, nx = src.shape
    sel_d, sel_s = [slice(None)], [slice(None)]
    for n, k in ((nz, s[2]), (ny, s[1]), (nx, s[0])):
        lo, hi = max(0, -k), min(n, n - k)
        if lo >= hi:
            return out
        sel_d.append(slice(lo, hi))
        sel_s.append(slice(lo + k, hi + k))
    out[tuple(sel_d)] = src[tuple(sel_s)]
    return out


def bench_shift(args, dev):
    from scsfm_hip import rolling
    dims = tuple(args.dims)
    nvox = dims[0] * dims[1] * dims[2]
    voxel = 16.0 / max(dims)
    vol = rolling.RollingVolume(dims, (-0.5 * dims[0] * voxel + 0.6, -0.5 * dims[1] * voxel, -1.0), voxel, device=dev)
    disp, images, c2w, K, max_depth = scene(64, 256, 832, dev, "drive")
    vol.integrate(disp, images, c2w, K, is_disp=True, max_depth=max_depth)
    del disp, images
    fused = vol.planes.clone()
    out = {"dims": list(dims), "voxels": nvox, "algorithmic_bytes": 40 * nvox, "shifts": []}
    for s in SHIFTS:
        vol.planes.copy_(fused)
        want = torch_shift(vol.planes, s)
        vol.move(s)
        same = bool(torch.equal(vol.planes.view(torch.int32), want.view(torch.int32)))
        del want
        t_hip, t_torch = [], []
        for k in range(args.reps + 1):      # (the first round warms both up)
            a = timed(lambda: vol.move(s))
            b = timed(lambda: torch_shift(vol.planes, s))
            if k:
                t_hip.append(a)
                t_torch.append(b)
        e = {"shift": list(s), "same_bits_as_torch": same, "hip": stats(t_hip), "torch": stats(t_torch)}
        e["hip"]["bytes_per_s"] = 40 * nvox / (e["hip"]["median_ms"] * 1e-3)
        e["hip"]["share_of_hbm_rate"] = e["hip"]["bytes_per_s"] / HBM_BYTES_PER_S
        e["ratio_torch_over_hip"] = e["torch"]["median_ms"] / e["hip"]["median_ms"]
        out["shifts"].append(e)
        print(f"shift {s}: {e['hip']['median_ms']:.3f} ms ({e['hip']['min_ms']:.3f} .. {e['hip']['max_ms']:.3f}), "
              f"{e['hip']['bytes_per_s'] / 1e12:.2f} TB/s; torch {e['torch']['median_ms']:.3f} ms; same bits: {same}", flush=True)
    # the leaving extraction, on the fused volume
    vol.planes.copy_(fused)
    del fused
    mw = 2.0
    full_points = int(vol.extract(mw)[0].shape[0])
    out["leaving"] = []
    for s in SHIFTS:
        points = int(vol.leaving(s, mw)[0].shape[0])
        t_leave, t_full = [], []
        for k in range(args.reps + 1):
            a = timed(lambda: vol.leaving(s, mw))
            b = timed(lambda: vol.extract(mw))
            if k:
                t_leave.append(a)
                t_full.append(b)
        e = {"shift": list(s), "keep_box": list(rolling.keep_box(dims, s)), "points": points, "points_of_the_volume": full_points,
             "leaving": stats(t_leave), "extract_whole": stats(t_full)}
        e["ratio_whole_over_leaving"] = e["extract_whole"]["median_ms"] / e["leaving"]["median_ms"]
        out["leaving"].append(e)
        print(f"leaving {s}: {e['leaving']['median_ms']:.3f} ms for {points} points; the whole volume "
              f"{e['extract_whole']['median_ms']:.3f} ms for {full_points}", flush=True)
    return out


def bench_follow(args, dev):
    from scsfm_hip import fusion, rolling
    P = FOLLOW
    F, bs = P["frames"], P["batch"]
    disp, images, c2w, K, _ = scene(F, 256, 832, dev, "drive")
    chain = c2w.cpu().numpy()
    trunc = fusion.TRUNC_VOXELS * P["voxel"]
    side = 8 * int(np.ceil((2.0 * (P["max_depth"] + trunc) / P["voxel"] + 2 * P["step"]) / 8.0))
    origin, dims = fusion.bounds_from_cameras(c2w, P["max_depth"], P["voxel"])
    base = torch.cuda.memory_allocated()

    def follow():
        spans, host = [], []
        vol = rolling.RollingVolume((side,) * 3, rolling.initial_origin(chain[bs // 2][:, 3], (side,) * 3, P["voxel"]),
                                    P["voxel"], device=dev)
        for k in range(0, F, bs):
            s = rolling.shift_for(chain[k + min(bs, F - k) // 2][:, 3], vol.origin0, vol.offset, vol.dims, vol.voxel, P["step"])
            if any(s):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                xyz, rgb = vol.shift(s, P["min_weight"])
                host.append((xyz.cpu(), rgb.cpu()))
                b.record()
                spans.append((a, b))
            vol.integrate(disp[k:k + bs], images[k:k + bs], c2w[k:k + bs], K, is_disp=True, max_depth=P["max_depth"])
        xyz, rgb = vol.extract(P["min_weight"])
        host.append((xyz.cpu(), rgb.cpu()))
        return spans, host, vol.offset

    def dense():
        vol = fusion.Volume(dims, origin, P["voxel"], device=dev)
        for k in range(0, F, bs):
            vol.integrate(disp[k:k + bs], images[k:k + bs], c2w[k:k + bs], K, is_disp=True, max_depth=P["max_depth"])
        xyz, rgb = vol.extract(P["min_weight"])
        return xyz.cpu(), rgb.cpu()

    peaks = {}
    for name, fn in (("follow", follow), ("dense", dense)):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        got = fn()
        torch.cuda.synchronize()
        peaks[name] = torch.cuda.max_memory_allocated() - base
        if name == "follow":
            spans, host, offset = got
            shifts, streamed, last = len(spans), sum(len(h[0]) for h in host[:-1]), len(host[-1][0])
        else:
            dense_points = len(got[0])
        del got
    t_follow, t_dense, t_shift = [], [], []
    for _ in range(args.reps):
        box = {}
        t_follow.append(timed(lambda: box.update(spans=follow()[0])))
        t_shift.append(sum(a.elapsed_time(b) for a, b in box["spans"]))
        t_dense.append(timed(dense))
    e = {"frames": F, "frame_size": [256, 832], "voxel": P["voxel"], "max_depth": P["max_depth"], "step": P["step"],
         "batch": bs, "min_weight": P["min_weight"], "window": [side] * 3, "window_bytes": 40 * side ** 3,
         "dense_dims": list(dims), "dense_bytes": 20 * dims[0] * dims[1] * dims[2], "follow": stats(t_follow),
         "dense": stats(t_dense), "shifts": shifts, "final_offset": list(offset), "in_shifts": stats(t_shift),
         "share_of_time_in_shifts": float(np.median(t_shift) / np.median(t_follow)), "peak_bytes_follow": peaks["follow"],
         "peak_bytes_dense": peaks["dense"], "points_streamed": streamed, "points_at_the_end": last, "points_dense": dense_points}
    e["ratio_dense_over_follow"] = e["dense"]["median_ms"] / e["follow"]["median_ms"]
    print(f"follow: {e['follow']['median_ms']:.1f} ms, peak {peaks['follow'] / 1e6:.0f} MB, {shifts} shifts "
          f"({100 * e['share_of_time_in_shifts']:.1f} % of the time), {streamed} + {last} points; dense {list(dims)}: "
          f"{e['dense']['median_ms']:.1f} ms, peak {peaks['dense'] / 1e6:.0f} MB, {dense_points} points", flush=True)
    return e


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--dims", type=int, nargs=3, default=[512, 128, 512])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rolling_bench.json"))
    args = ap.parse_args(argv)
    if args.reps < 15:
        raise SystemExit("--reps: at least 15")
    if not torch.cuda.is_available():
        raise SystemExit("bench_rolling.py needs a HIP device")
    from scsfm_hip import _lib
    _lib.get_roll()  # (a missing library is an error before anything is timed)
    dev = torch.device("cuda")
    result = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "hbm_bytes_per_s": HBM_BYTES_PER_S}
    result["volume"] = bench_shift(args, dev)
    torch.cuda.empty_cache()
    result["follow"] = bench_follow(args, dev)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps({"device": result["device"], "reps": args.reps, "out": args.out}))


if __name__ == "__main__":
    main()
