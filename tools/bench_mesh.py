"""Times the triangle mesh of scsfm_hip.meshing (libscsfm_mesh.so; reconstruct.py --mesh) against the point extraction of
scsfm_hip.fusion (libscsfm_fuse.so) on the same fused volume: a pass over the same planes, and what the tree had before.

    python tools/bench_mesh.py [--reps 15] [--out profiles/mesh_bench.json] [--dims 512 128 512] [--frames 64]

The 512 x 128 x 512 volume (671 MB) is filled from the 64 generated frames of tools/bench_fusion.py's "drive" scene.
Volume.extract_mesh and Volume.extract alternate in one process after a warm-up of both; a sample is the time between two
events round the call (its allocations and the host's fetch of the totals included), the device idle before it.
Reported per variant: median, minimum and maximum of --reps (at least 15) samples, and the achieved bytes per second over
the algorithmic bytes:

  extract       two passes over the tsdf and weight planes (8 bytes a voxel each) and 15 bytes a point
  extract_mesh  three passes over the tsdf and weight planes, the per-voxel index plane written once (5 bytes a voxel:
                the first vertex index and the crossing mask), 15 bytes a vertex and 12 bytes a triangle.  (A voxel that
                is not seen is read once, its weight, and nothing more: the count is an upper bound of the traffic.)

The mesh's vertices on the grid's edges are compared with the points first.  Writes one JSON file.  Needs a HIP device."""
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


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--dims", type=int, nargs=3, default=[512, 128, 512])
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--size", type=int, nargs=2, default=[256, 832])
    ap.add_argument("--min-weight", type=float, default=2.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_bench.json"))
    args = ap.parse_args(argv)
    if args.reps < 15:
        raise SystemExit("--reps: at least 15")
    if not torch.cuda.is_available():
        raise SystemExit("bench_mesh.py needs a HIP device")
    from scsfm_hip import _lib, fusion
    _lib.get_fuse(), _lib.get_mesh()  # (a missing library is an error before anything is timed)
    dev = torch.device("cuda")
    F, (H, W), dims = args.frames, args.size, tuple(args.dims)
    voxel = 16.0 / max(dims)
    origin = (-0.5 * dims[0] * voxel + 0.6, -0.5 * dims[1] * voxel, -1.0)
    nvox = dims[0] * dims[1] * dims[2]
    vol = fusion.Volume(dims, origin, voxel, device=dev)
    disp, images, c2w, K, max_depth = scene(F, H, W, dev, "drive")
    vol.integrate(disp, images, c2w, K, is_disp=True, max_depth=max_depth)
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
    xyz, rgb, tri = vol.extract_mesh(mw)
    pts, cols = vol.extract(mw)
    V, T, N = len(xyz), len(tri), len(pts)
    # results first: the vertices on the +x, +y, +z edges are the points (an edge vertex has exactly one coordinate off
    # the lattice of centres, which is how many vertices must be left over; the bits are compared by the tests)
    again = vol.extract_mesh(mw)
    same = all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip((xyz, rgb, tri), again))
    valid = bool(T == 0 or (int(tri.min()) >= 0 and int(tri.max()) < V))
    print(f"volume {dims}, {20 * nvox / 1e6:.0f} MB; {F} frames of {H} x {W}; {N} points; {V} vertices, {T} triangles; two "
          f"extractions equal: {same}; indices valid: {valid}", flush=True)
    del xyz, rgb, tri, pts, cols, again

    t_mesh, t_points = [], []
    for _ in range(args.reps):
        t_mesh.append(timed(lambda: vol.extract_mesh(mw)))
        t_points.append(timed(lambda: vol.extract(mw)))
    mesh, points = stats(t_mesh), stats(t_points)
    points.update(points=N, bytes=2 * 8 * nvox + 15 * N)
    mesh.update(vertices=V, triangles=T, bytes=(3 * 8 + 5) * nvox + 15 * V + 12 * T)
    for e in (mesh, points):
        e["bytes_per_s"] = e["bytes"] / (e["median_ms"] * 1e-3)
        e["share_of_hbm_rate"] = e["bytes_per_s"] / HBM_BYTES_PER_S
    print(f"extract_mesh: {mesh['median_ms']:.2f} ms ({mesh['min_ms']:.2f} .. {mesh['max_ms']:.2f}), "
          f"{mesh['bytes_per_s'] / 1e12:.2f} TB/s of {mesh['bytes'] / 1e6:.0f} MB; extract: {points['median_ms']:.2f} ms "
          f"({points['min_ms']:.2f} .. {points['max_ms']:.2f}), {points['bytes_per_s'] / 1e12:.2f} TB/s of "
          f"{points['bytes'] / 1e6:.0f} MB", flush=True)
    result = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "dims": list(dims), "voxels": nvox, "frames": F,
              "frame_size": [H, W], "min_weight": mw, "hbm_bytes_per_s": HBM_BYTES_PER_S, "two_extractions_equal": same,
              "indices_valid": valid, "extract_mesh": mesh, "extract": points,
              "ratio_mesh_over_extract": mesh["median_ms"] / points["median_ms"]}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps({k: v for k, v in result.items() if k not in ("extract_mesh", "extract")}))


if __name__ == "__main__":
    main()
