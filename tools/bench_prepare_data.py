"""Times the per-frame work of data/prepare_train_data.py on a generated KITTI-sized scene (no dataset needed): 100
frames of 375 x 1242 resized to 128 x 416 and to 256 x 832, 100 Velodyne scans of ~120,000 points.

    python tools/bench_prepare_data.py [--frames 100] [--out profiles/prepare_data_bench.json]

  kernels    scsfm_hip.prepare.resize_u8 and velodyne_depth with their inputs already on the device (one call for all
             frames; median of the repetitions, timed with events after a warm-up call)
  host       PIL's Image.resize(BILINEAR) and a numpy restatement of generate_depth_map, on 16 host threads
  pipeline   PNG file -> decode -> resize -> JPEG file (+ scan file -> depth map -> .npy), through the GPU in batches of
             32 with 16 decode / encode threads as the command-line program does it, and on the host alone; with the
             share of the host-only stages (decode, encode), which no kernel shortens
Writes one JSON file.  Needs a HIP device."""
from __future__ import annotations

import argparse
import json
import os
import shutil
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sc-sfmlearner-release_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402
from PIL import Image  # noqa: E402

from scsfm_hip import prepare  # noqa: E402

THREADS, BATCH = 16, 32
RAW_H, RAW_W = 375, 1242
P_RECT = np.array([[721.5377, 0, 609.5593, 44.85728], [0, 721.5377, 172.854, 0.2163791], [0, 0, 1, 0.002745884]])
VELO_R = np.array([[7.533745e-03, -9.999714e-01, -6.166020e-04], [1.480249e-02, 7.280733e-04, -9.998902e-01],
                   [9.998621e-01, 7.523790e-03, 1.480755e-02]])
VELO_T = np.array([-4.069766e-03, -7.631618e-02, -2.717806e-01])


def numpy_depth(velo, P, h, w):
    """generate_depth_map restated with numpy (np.unique instead of the Counter loop)."""
    velo = velo.copy()
    velo[:, 3] = 1
    velo = velo[velo[:, 0] >= 0]
    pts = np.dot(P, velo.T).T
    with np.errstate(all="ignore"):
        pts[:, :2] = pts[:, :2] / pts[:, -1:]
    pts[:, 0] = np.round(pts[:, 0]) - 1
    pts[:, 1] = np.round(pts[:, 1]) - 1
    pts = pts[(pts[:, 0] >= 0) & (pts[:, 1] >= 0) & (pts[:, 0] < w) & (pts[:, 1] < h)]
    depth = np.zeros((h, w), np.float32)
    ui, vi = pts[:, 0].astype(np.int64), pts[:, 1].astype(np.int64)
    depth[vi, ui] = pts[:, 2]
    key = vi * (w - 1) + ui - 1
    _, first, inverse, count = np.unique(key, return_index=True, return_inverse=True, return_counts=True)
    zmin = np.full(len(first), np.inf)
    np.minimum.at(zmin, inverse, pts[:, 2])
    dup = count > 1
    depth[vi[first[dup]], ui[first[dup]]] = zmin[dup]
    depth[depth < 0] = 0
    return depth


def stats(ms):
    return {"median_ms": float(np.median(ms)), "min_ms": float(np.min(ms)), "reps": len(ms)}


def gpu_time(fn, reps=7):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return stats(ms)


def wall_time(fn, reps=3):
    ms = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t) * 1e3)
    return stats(ms)


def make_scan(rng, n=120000):
    """A ring-like cloud: most of it around the sensor, about a fifth inside the camera's field of view."""
    ang = rng.uniform(-np.pi, np.pi, n)
    dist = rng.uniform(3, 70, n)
    return np.stack([dist * np.cos(ang), dist * np.sin(ang), rng.uniform(-2.5, 1.0, n), rng.uniform(0, 1, n)],
                    1).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prepare_data_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_prepare_data.py needs a HIP device")
    dev, F = torch.device("cuda"), args.frames
    rng = np.random.default_rng(0)
    # smooth frames (a blurred noise field compresses like a photograph, unlike white noise) plus a little grain
    base = rng.integers(0, 256, (8, RAW_H // 8 + 1, RAW_W // 8 + 1, 3), dtype=np.uint8)
    frames = np.stack([np.asarray(Image.fromarray(base[k % 8]).resize((RAW_W, RAW_H), Image.BICUBIC)) for k in range(F)])
    frames = np.clip(frames.astype(np.int16) + rng.integers(-6, 7, frames.shape, dtype=np.int16), 0, 255).astype(np.uint8)
    scans = [make_scan(rng) for _ in range(F)]
    result = {"device": torch.cuda.get_device_name(0), "frames": F, "raw_size": [RAW_H, RAW_W],
              "points_per_scan": len(scans[0]), "host_threads": THREADS, "batch": BATCH}
    pool = ThreadPoolExecutor(THREADS)
    tmp = tempfile.mkdtemp(prefix="prepare_bench_")
    try:
        png = [os.path.join(tmp, f"{k:010d}.png") for k in range(F)]
        binf = [os.path.join(tmp, f"{k:010d}.bin") for k in range(F)]
        list(pool.map(lambda a: Image.fromarray(a[1]).save(a[0]), zip(png, frames)))
        for f, s in zip(binf, scans):
            s.tofile(f)
        d_frames = torch.from_numpy(frames).to(dev)
        d_points = torch.from_numpy(np.concatenate(scans)).to(dev)
        d_off = torch.from_numpy(np.concatenate([[0], np.cumsum([len(s) for s in scans])]).astype(np.int32)).to(dev)
        for h, w in ((128, 416), (256, 832)):
            P_rect = P_RECT.copy()
            P_rect[0] *= w / RAW_W
            P_rect[1] *= h / RAW_H
            P = prepare.velo_projection(P_rect, np.eye(3), VELO_R, VELO_T, 1)
            d_P = torch.from_numpy(np.repeat(P[None], F, 0)).to(dev)
            r = {}
            r["resize_u8_gpu"] = gpu_time(lambda: prepare.resize_u8(d_frames, h, w))
            r["resize_pil_16_threads"] = wall_time(lambda: list(pool.map(
                lambda a: np.asarray(Image.fromarray(a).resize((w, h), Image.BILINEAR)), frames)))
            r["velodyne_depth_gpu"] = gpu_time(lambda: prepare.velodyne_depth(d_points, d_off, d_P, h, w, (float(w), float(h))))
            r["velodyne_depth_numpy_16_threads"] = wall_time(lambda: list(pool.map(lambda s: numpy_depth(s, P, h, w), scans)))
            got = prepare.velodyne_depth(d_points[:len(scans[0])], d_off[:2], d_P[:1], h, w, (float(w), float(h)))[0].cpu().numpy()
            want = numpy_depth(scans[0], P, h, w)
            r["depth_entries_differing_from_numpy"] = int((got != want).sum())
            r["resize_bytes_differing_from_pil"] = int((prepare.resize_u8(d_frames[:1], h, w)[0].cpu().numpy() != np.asarray(
                Image.fromarray(frames[0]).resize((w, h), Image.BILINEAR))).sum())

            out_dir = os.path.join(tmp, f"out_{h}")
            os.makedirs(out_dir, exist_ok=True)
            decode = lambda f: np.asarray(Image.open(f))
            encode = lambda a: Image.fromarray(a[1]).save(os.path.join(out_dir, f"{a[0]:010d}.jpg"))
            load = lambda f: np.fromfile(f, np.float32).reshape(-1, 4)

            def gpu_pipeline():
                for s in range(0, F, BATCH):
                    idx = range(s, min(s + BATCH, F))
                    imgs = list(pool.map(decode, [png[k] for k in idx]))
                    small = prepare.resize_u8(torch.from_numpy(np.stack(imgs)).to(dev), h, w).cpu().numpy()
                    list(pool.map(encode, zip(idx, small)))
                    sc = list(pool.map(load, [binf[k] for k in idx]))
                    off = torch.from_numpy(np.concatenate([[0], np.cumsum([len(x) for x in sc])]).astype(np.int32)).to(dev)
                    depth = prepare.velodyne_depth(torch.from_numpy(np.concatenate(sc)).to(dev), off, d_P[:len(sc)], h, w,
                                                   (float(w), float(h))).cpu().numpy()
                    for k, d in zip(idx, depth):
                        np.save(os.path.join(out_dir, f"{k:010d}.npy"), d)

            def host_frame(k):
                encode((k, np.asarray(Image.fromarray(decode(png[k])).resize((w, h), Image.BILINEAR))))
                np.save(os.path.join(out_dir, f"{k:010d}.npy"), numpy_depth(load(binf[k]), P, h, w))

            r["pipeline_gpu"] = wall_time(gpu_pipeline)
            r["pipeline_host_16_threads"] = wall_time(lambda: list(pool.map(host_frame, range(F))))
            r["png_decode_16_threads"] = wall_time(lambda: list(pool.map(decode, png)))
            small = prepare.resize_u8(d_frames, h, w).cpu().numpy()
            r["jpeg_encode_16_threads"] = wall_time(lambda: list(pool.map(encode, enumerate(small))))
            r["decode_plus_encode_share_of_pipeline_gpu"] = (
                r["png_decode_16_threads"]["median_ms"] + r["jpeg_encode_16_threads"]["median_ms"]) / r["pipeline_gpu"]["median_ms"]
            result[f"{h}x{w}"] = r
            print(f"{h}x{w}", json.dumps(r), flush=True)
    finally:
        pool.shutdown()
        shutil.rmtree(tmp, ignore_errors=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
