"""Times the TSDF fusion of scsfm_hip.fusion (libscsfm_fuse.so; reconstruct.py) against a torch restatement of the same
update on the device -- what a user would otherwise write.

    python tools/bench_fusion.py [--reps 15] [--out profiles/fusion_bench.json] [--dims 512 128 512] [--frames 64]

A 512 x 128 x 512 volume (671 MB, 16 x 4 x 16 units) and 64 frames of 256 x 832 with their images, all on the device, in
two scenes: "covering" -- the camera stands 10 units in front of the box and looks through it at a surface near its far
end, so every frame updates nearly every voxel: the case the frames-per-launch design is for -- and "drive" -- the camera
moves forward through the box and turns slowly, looking at a surface 1.5 to 6.5 units away, as reconstruct.py's box (the
cameras' box grown by the depth limit) leaves it: most tiles lie outside every frustum.  Measured per scene, alternating
in one process after a warm-up of every variant:

  integrate  all frames into an emptied volume at 1, 4, 8 and 16 frames per launch; a sample is the time between two
             events round the launches, the device idle before the first.  Reported per variant: median, minimum and
             maximum of --reps (at least 15) samples, the time per frame, and the volume's traffic as if every tile moved
             in every launch (40 bytes per voxel and launch: an upper bound, since tiles outside every frustum of a launch
             move nothing -- "tiles_seen" is the share of the 32 x 8 x 4 tiles with a seen voxel at the end) over the
             median, as bytes per second and as a share of the 8 TB/s HBM rate.
  torch      the same update in torch operations, --torch-frames frames (default 4: every frame reads and writes the
             whole volume several times over), per frame.
  extract    count + extract of the fused volume; its two passes read the tsdf and weight planes (8 bytes per voxel each).

The fused volumes of all variants are compared first: the launches' split leaves the same bits, and the torch restatement
agrees to rounding where it was run.  Writes one JSON file.  Needs a HIP device."""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sc-sfmlearner-release_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

HBM_BYTES_PER_S = 8.0e12
FRAMES_PER_LAUNCH = (1, 4, 8, 16)


def stats(v):
    return {"median_ms": float(np.median(v)), "min_ms": float(np.min(v)), "max_ms": float(np.max(v)),
            "runs_ms": [round(float(x), 4) for x in v]}


def scene(F, H, W, dev, kind="drive"):
    """-> disparity [F, 1, H, W], images [F, 3, H, W], c2w float64 [F, 3, 4], K [3, 3], max_depth.  "drive": forward
    through the box with a slow turn, the surface 1.5 to 6.5 away; "covering": 10 in front of the box (whose z starts at
    -1), creeping forward, the surface 23.5 to 25 away, near the far end of the box"""
    g = torch.Generator().manual_seed(0)
    yy, xx = torch.meshgrid(torch.linspace(0, 1, H), torch.linspace(0, 1, W), indexing="ij")
    covering = kind == "covering"
    far, amp = (24.0, 0.5) if covering else (3.0, 2.0)
    depth = torch.stack([far + amp * torch.sin(3 * xx + 0.1 * k) * torch.cos(2 * yy) + 0.75 * amp * yy for k in range(F)])
    disp = (1.0 / depth).unsqueeze(1).contiguous()
    images = torch.randn((F, 3, H, W), generator=g)
    c2w = np.zeros((F, 3, 4))
    for k in range(F):
        a = 0.0 if covering else 0.004 * k
        c2w[k, :, :3] = [[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]
        c2w[k, :, 3] = [0.6 + 0.002 * k, 0.0, -11.0 + 0.01 * k] if covering else [0.02 * k, 0.0, 0.08 * k]
    K = torch.tensor([[0.58 * W, 0, 0.5 * W], [0, 1.92 * H, 0.5 * H], [0, 0, 1]])
    return disp.to(dev), images.to(dev), torch.from_numpy(c2w).to(dev), K.to(dev), (30.0 if covering else 8.0)


def torch_integrate(planes, origin, voxel, trunc, max_weight, disp, images, cam, max_depth):
    """the header's update in torch operations, one frame after another, on the whole volume"""
    _, nz, ny, nx = planes.shape
    dev = planes.device
    ax = lambda o, n: o + (torch.arange(n, device=dev, dtype=torch.float32) + 0.5) * voxel  # noqa: E731
    x, y, z = ax(origin[0], nx)[None, None, :], ax(origin[1], ny)[None, :, None], ax(origin[2], nz)[:, None, None]
    H, W = disp.shape[-2:]
    t, w = planes[0], planes[1]
    for f in range(disp.shape[0]):
        c = cam[f].tolist()
        qx = c[0] * x + c[1] * y + c[2] * z + c[9]
        qy = c[3] * x + c[4] * y + c[5] * z + c[10]
        qz = c[6] * x + c[7] * y + c[8] * z + c[11]
        a, b = c[12] * qx / qz + c[14] + 0.5, c[13] * qy / qz + c[15] + 0.5
        ok = (qz > 0) & (a >= 0) & (a < W) & (b >= 0) & (b < H)
        px, py = torch.where(ok, a, 0).long(), torch.where(ok, b, 0).long()
        d = 1.0 / disp[f, 0][py, px]
        sdf = d - qz
        ok &= (d > 0) & (d <= max_depth) & (sdf >= -trunc)
        w1 = w + 1
        t.copy_(torch.where(ok, (t * w + torch.clamp(sdf / trunc, max=1.0)) / w1, t))
        for ch in range(3):
            col = images[f, ch][py, px] * 0.225 + 0.45
            planes[2 + ch].copy_(torch.where(ok, (planes[2 + ch] * w + col) / w1, planes[2 + ch]))
        w.copy_(torch.where(ok, torch.clamp(w1, max=max_weight), w))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--dims", type=int, nargs=3, default=[512, 128, 512])
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--size", type=int, nargs=2, default=[256, 832])
    ap.add_argument("--torch-frames", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fusion_bench.json"))
    args = ap.parse_args(argv)
    if args.reps < 15:
        raise SystemExit("--reps: at least 15")
    if not torch.cuda.is_available():
        raise SystemExit("bench_fusion.py needs a HIP device")
    from scsfm_hip import _lib, fusion
    _lib.get_fuse()  # (a missing library is an error before anything is timed)
    dev = torch.device("cuda")
    F, (H, W), dims = args.frames, args.size, tuple(args.dims)
    voxel = 16.0 / max(dims)
    origin = (-0.5 * dims[0] * voxel + 0.6, -0.5 * dims[1] * voxel, -1.0)
    nvox = dims[0] * dims[1] * dims[2]
    vols = {n: fusion.Volume(dims, origin, voxel, device=dev, frames_per_launch=n) for n in FRAMES_PER_LAUNCH}
    ref = torch.zeros_like(vols[1].planes)

    def measure(kind):
        disp, images, c2w, K, max_depth = scene(F, H, W, dev, kind)

        def timed(fn):
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            return a.elapsed_time(b)

        for n in FRAMES_PER_LAUNCH:
            vols[n].planes.zero_()
        ref.zero_()
        cam = fusion.cameras(c2w, K)
        tf = min(args.torch_frames, F)

        def run_hip(n):
            vols[n].integrate(disp, images, c2w, K, is_disp=True, max_depth=max_depth)

        def run_torch():
            torch_integrate(ref, vols[1].origin, vols[1].voxel, vols[1].trunc, 64.0, disp[:tf], images[:tf], cam, max_depth)

        # results first: the same bits at every split; the torch restatement to rounding on its frames
        for n in FRAMES_PER_LAUNCH:
            run_hip(n)
        same = all(torch.equal(vols[1].planes, vols[n].planes) for n in FRAMES_PER_LAUNCH[1:])
        check = fusion.Volume(dims, origin, voxel, device=dev, frames_per_launch=tf)
        check.integrate(disp[:tf], images[:tf], c2w[:tf], K, is_disp=True, max_depth=max_depth)
        run_torch()
        agree = float(((check.planes - ref).abs() <= 1e-4).float().mean())
        del check
        tiles = vols[1].weight
        pad = [(-s) % t for s, t in zip(tiles.shape, (4, 8, 32))]
        tiles = torch.nn.functional.pad(tiles, (0, pad[2], 0, pad[1], 0, pad[0]))
        tiles = tiles.reshape(tiles.shape[0] // 4, 4, tiles.shape[1] // 8, 8, tiles.shape[2] // 32, 32).amax(dim=(1, 3, 5))
        tiles_seen = float((tiles > 0).float().mean())
        print(f"{kind}: volume {dims}, {20 * nvox / 1e6:.0f} MB; {F} frames of {H} x {W}; same bits at every split: {same}; torch "
              f"agrees on {100 * agree:.3f} % of the entries; tiles seen {100 * tiles_seen:.1f} %", flush=True)

        t = {n: [] for n in FRAMES_PER_LAUNCH}
        t_torch, t_extract = [], []
        for _ in range(args.reps):
            for n in FRAMES_PER_LAUNCH:
                vols[n].planes.zero_()
                t[n].append(timed(lambda: run_hip(n)))
            ref.zero_()
            t_torch.append(timed(run_torch))
            t_extract.append(timed(lambda: vols[8].extract(2.0)))
        n_points = int(vols[8].extract(2.0)[0].shape[0])

        entries = []
        for n in FRAMES_PER_LAUNCH:
            launches = -(-F // n)
            e = {"frames_per_launch": n, "launches": launches, **stats(t[n])}
            e["ms_per_frame"] = e["median_ms"] / F
            e["volume_bytes_upper_bound"] = launches * 40 * nvox
            e["upper_bound_bytes_per_s"] = e["volume_bytes_upper_bound"] / (e["median_ms"] * 1e-3)
            e["upper_bound_share_of_hbm_rate"] = e["upper_bound_bytes_per_s"] / HBM_BYTES_PER_S
            entries.append(e)
            print(f"integrate, {n:2d} frames a launch: {e['median_ms']:.2f} ms ({e['min_ms']:.2f} .. {e['max_ms']:.2f}), "
                  f"{e['ms_per_frame']:.3f} ms a frame, at most {e['upper_bound_bytes_per_s'] / 1e12:.2f} TB/s", flush=True)
        tt = stats(t_torch)
        tt["frames"] = tf
        tt["ms_per_frame"] = tt["median_ms"] / tf
        ex = stats(t_extract)
        ex["points"] = n_points
        ex["bytes"] = 2 * 8 * nvox
        ex["bytes_per_s"] = ex["bytes"] / (ex["median_ms"] * 1e-3)
        ex["share_of_hbm_rate"] = ex["bytes_per_s"] / HBM_BYTES_PER_S
        best = min(entries, key=lambda e: e["median_ms"])
        print(f"torch restatement: {tt['ms_per_frame']:.2f} ms a frame ({tt['min_ms'] / tf:.2f} .. {tt['max_ms'] / tf:.2f}); "
              f"extract: {ex['median_ms']:.2f} ms for {n_points} points, {ex['bytes_per_s'] / 1e12:.2f} TB/s", flush=True)
        return {"scene": kind, "max_depth": max_depth, "same_bits_at_every_split": same, "torch_agrees_share": agree,
                "tiles_seen": tiles_seen, "integrate": entries, "torch": tt, "extract": ex,
                "fastest_frames_per_launch": best["frames_per_launch"],
                "ratio_torch_over_hip_per_frame": tt["ms_per_frame"] / best["ms_per_frame"]}

    scenes = [measure(kind) for kind in ("covering", "drive")]
    result = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "dims": list(dims), "voxels": nvox,
              "frames": F, "frame_size": [H, W], "hbm_bytes_per_s": HBM_BYTES_PER_S,
              "default_frames_per_launch": fusion.FRAMES_PER_LAUNCH, "scenes": scenes}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps({k: v for k, v in result.items() if k != "scenes"}))


if __name__ == "__main__":
    main()
