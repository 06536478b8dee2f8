"""Times the ray cast of scsfm_hip.raycast (libscsfm_cast.so; reconstruct.py --render) with and without its brick cull,
the brick mask alone, and Volume.extract_mesh beside them for scale, all on the same fused volume.

    python tools/bench_raycast.py [--reps 15] [--out profiles/raycast_bench.json] [--dims 512 128 512] [--frames 64]

The 512 x 128 x 512 volume (671 MB) is filled from the 64 generated frames of tools/bench_fusion.py's "drive" scene, and
the 64 fusing poses are cast at 256 x 832 with a step of one voxel from 0 to max_depth + trunc, all outputs on.
cast (the mask built before, handed in), cast with cull=False, brick_mask and extract_mesh alternate in one process after
a warm-up of each; a sample is the time between two events round the call (its allocations included), the device idle
before it.  Reported per variant: median, minimum and maximum of --reps (at least 15) samples, and the achieved bytes per
second over the algorithmic bytes:

  cast          20 bytes a pixel written (depth 4, normal 12, colour 3, shade 1), the view records, and -- as the floor
                of what must come from memory -- the tsdf and weight planes once (8 bytes a voxel; with the cull, the
                mask's bytes as well).  The gathers themselves are served by the caches: the figure that describes them
                is samples per second (V H W n_steps samples, each eight tsdf and eight weight corners without the cull).
  brick_mask    the tsdf and weight planes once (8 bytes a voxel) and one byte a brick written; the kernel itself reads
                (9 / 8)^2 of that, the bricks' ranges overlapping by one voxel in y and z.

The two casts are compared bit for bit first.  Writes one JSON file.  Needs a HIP device."""
from __future__ import annotations

import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sc-sfmlearner-release_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

from bench_fusion import HBM_BYTES_PER_S, scene, stats  # noqa: E402


# Forms of the march that were measured against the shipped one with this tool on an MI355X (medians of 15, the default
# volume and views) and lost; a run of the tool copies the record into its file, it does not measure them again.
OTHER_FORMS = {
    "box_exit": {"what": "end a ray once it has been in range of the volume and is not any more (exact: the samples in "
                         "range are consecutive), carrying the next sample's cell instead of recomputing the "
                         "evaluated sample's",
                 "cast_median_ms": 7.226, "cast_no_cull_median_ms": 10.044,
                 "shipped_form_same_session": {"cast_median_ms": 6.647, "cast_no_cull_median_ms": 9.963}, "kept": False},
    "brick_exit_jump": "not tried: the kernel steps one sample at a time and only skips the fetches",
}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--dims", type=int, nargs=3, default=[512, 128, 512])
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--size", type=int, nargs=2, default=[256, 832])
    ap.add_argument("--min-weight", type=float, default=2.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "raycast_bench.json"))
    args = ap.parse_args(argv)
    if args.reps < 15:
        raise SystemExit("--reps: at least 15")
    if not torch.cuda.is_available():
        raise SystemExit("bench_raycast.py needs a HIP device")
    from scsfm_hip import _lib, fusion, raycast
    _lib.get_fuse(), _lib.get_mesh(), _lib.get_cast()  # (a missing library is an error before anything is timed)
    dev = torch.device("cuda")
    F, (H, W), dims = args.frames, args.size, tuple(args.dims)
    voxel = 16.0 / max(dims)
    origin = (-0.5 * dims[0] * voxel + 0.6, -0.5 * dims[1] * voxel, -1.0)
    nvox = dims[0] * dims[1] * dims[2]
    vol = fusion.Volume(dims, origin, voxel, device=dev)
    disp, images, c2w, K, max_depth = scene(F, H, W, dev, "drive")
    vol.integrate(disp, images, c2w, K, is_disp=True, max_depth=max_depth)
    pred = 1.0 / disp[:, 0]
    del disp, images

    def timed(fn):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    mw = args.min_weight
    far = max_depth + vol.trunc
    n_steps = int(math.ceil(far / vol.voxel))
    mask = raycast.brick_mask(vol, mw)
    marked = int(mask.sum())

    def cast(**kw):
        return vol.raycast(c2w, K, (H, W), 0.0, far, min_weight=mw, **kw)

    # results first: the cull changes no bit
    culled, plain = cast(mask=mask), cast(cull=False)
    same = all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(culled, plain))
    hit = culled.depth > 0
    both = hit & (pred <= max_depth)
    share = float(hit.double().mean())
    agree = float(((pred - culled.depth).abs() / culled.depth)[both].double().mean()) if bool(both.any()) else float("nan")
    print(f"volume {dims}, {20 * nvox / 1e6:.0f} MB; {F} views of {H} x {W}, {n_steps} steps a ray; {marked} of "
          f"{mask.numel()} bricks marked; with and without the cull equal: {same}; {share:.4f} of the pixels with a hit; "
          f"mean |pred - fused| / fused {agree:.5f}", flush=True)
    del culled, plain, hit, both, pred
    vol.extract_mesh(mw)

    runs = {"cast": [], "cast_no_cull": [], "brick_mask": [], "extract_mesh": []}
    for _ in range(args.reps):
        runs["cast"].append(timed(lambda: cast(mask=mask)))
        runs["cast_no_cull"].append(timed(lambda: cast(cull=False)))
        runs["brick_mask"].append(timed(lambda: raycast.brick_mask(vol, mw)))
        runs["extract_mesh"].append(timed(lambda: vol.extract_mesh(mw)))
    out = {k: stats(v) for k, v in runs.items()}
    pixels = F * H * W
    out["cast"]["bytes"] = 20 * pixels + 64 * F + 8 * nvox + mask.numel()
    out["cast_no_cull"]["bytes"] = 20 * pixels + 64 * F + 8 * nvox
    out["brick_mask"]["bytes"] = 8 * nvox + mask.numel()
    for k in ("cast", "cast_no_cull", "brick_mask"):
        e = out[k]
        e["bytes_per_s"] = e["bytes"] / (e["median_ms"] * 1e-3)
        e["share_of_hbm_rate"] = e["bytes_per_s"] / HBM_BYTES_PER_S
    for k in ("cast", "cast_no_cull"):
        out[k]["samples"] = pixels * n_steps
        out[k]["samples_per_s"] = pixels * n_steps / (out[k]["median_ms"] * 1e-3)
        out[k]["ms_per_view"] = out[k]["median_ms"] / F
    for k, e in out.items():
        print(f"{k}: {e['median_ms']:.3f} ms ({e['min_ms']:.3f} .. {e['max_ms']:.3f})", flush=True)
    result = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "dims": list(dims), "voxels": nvox, "views": F,
              "view_size": [H, W], "min_weight": mw, "near": 0.0, "far": far, "step": vol.voxel, "n_steps": n_steps,
              "bricks": mask.numel(), "bricks_marked": marked, "hbm_bytes_per_s": HBM_BYTES_PER_S,
              "cull_changes_no_bit": same, "share_of_pixels_with_a_hit": share, "mean_rel_depth_difference": agree, **out,
              "ratio_no_cull_over_cull": out["cast_no_cull"]["median_ms"] / out["cast"]["median_ms"],
              "other_forms": OTHER_FORMS}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps({k: v for k, v in result.items() if k not in out}))


if __name__ == "__main__":
    main()
