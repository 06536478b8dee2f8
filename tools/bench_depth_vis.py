"""Times the device path of eval_depth.py --vis_dir for a KITTI-Eigen-sized set (no dataset needed): 697 generated
float64 predictions of 256 x 832, each resized to a 375 x 1242 ground-truth size, scaled, ranged and coloured into a
[750, 1242, 3] canvas under its photograph.  PNG encoding is not part of it.

    python tools/bench_depth_vis.py [--maps 697] [--out profiles/depth_vis_bench.json]

  device     scsfm_hip.depth_vis.composites over the set in chunks of 2^24 ground-truth pixels, predictions and
             photographs already on the device (median of the repetitions, timed with events after a warm-up pass),
             and the same followed by the canvases' copies back to the host
  host       the reference's chain per image -- inverse-depth resize (the numpy restatement of INTER_LINEAR), ratio,
             np.percentile, matplotlib's Normalize and magma, the canvas -- on 16 host threads
The first canvases of the two paths are compared byte for byte.  Writes one JSON file.  Needs a HIP device and
matplotlib."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
import types
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sc-sfmlearner-release_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from scsfm_hip import depth_vis  # noqa: E402

THREADS = 16
H, W = 375, 1242
h, w = 256, 832
CHUNK_PIXELS = 1 << 24


def host_canvas(pred, ratio, photo):
    """One prediction -> its canvas, with numpy and matplotlib as the reference's main does it."""
    import matplotlib as mpl
    import matplotlib.cm as cm
    from depth_eval_oracle import resize_linear
    depth = 1 / (resize_linear(1 / (pred + 1e-6), W, H) + 1e-6) * ratio
    inv = 1 / (depth + 1e-6)
    norm = mpl.colors.Normalize(vmin=inv.min(), vmax=np.percentile(inv, 95))
    vis = (cm.ScalarMappable(norm=norm, cmap='magma').to_rgba(inv)[:, :, :3] * 255).astype(np.uint8)
    cat = np.zeros((2 * H, W, 3))
    cat[:H] = photo
    cat[H:] = vis
    return cat.astype(np.uint8)


def median_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        fn()
        end.record()
        end.synchronize()
        times.append(start.elapsed_time(end))
    return float(np.median(times)), [float(t) for t in times]


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--maps", type=int, default=697)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-maps", type=int, default=64, help="maps the host chain is timed on (scaled to --maps)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "depth_vis_bench.json"))
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_depth_vis.py needs a HIP device")
    rng = np.random.default_rng(0)
    N = args.maps
    ramp = np.linspace(1.0, 0.05, h)[:, None]
    pred = np.stack([0.02 + ramp * rng.uniform(0.5, 2.0) * (0.8 + 0.4 * rng.random((h, w))) for _ in range(N)])
    ratios = rng.uniform(20.0, 40.0, N)
    photo = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    res = types.SimpleNamespace(ratio=ratios, evaluated=np.ones(N, bool))
    gts = [np.empty((H, W), np.float32)] * N  # only the sizes and the dtype are read for KITTI
    d_pred = torch.from_numpy(pred).cuda()
    d_photo = torch.from_numpy(photo).cuda()
    per = max(1, CHUNK_PIXELS // (H * W))

    def device(copy=False):
        first = None
        for k0 in range(0, N, per):
            n = min(per, N - k0)
            c = depth_vis.composites(res, d_pred, gts, "kitti", [d_photo] * n, first=k0)
            if copy:
                c = [x.cpu() for x in c]
            first = first or c
        return first

    device_ms, device_runs = median_ms(device, args.reps)
    copies_ms, copies_runs = median_ms(lambda: device(True), args.reps)

    m = min(args.host_maps, N)
    t0 = time.perf_counter()
    with ThreadPoolExecutor(THREADS) as pool:
        host = list(pool.map(lambda i: host_canvas(pred[i], ratios[i], photo), range(m)))
    host_ms = (time.perf_counter() - t0) * 1e3

    k = min(4, m)
    got = [c.cpu().numpy() for c in device()[:k]]
    equal = all(np.array_equal(got[i], host[i]) for i in range(k))
    result = {"maps": N, "pred": [h, w], "gt": [H, W], "pred_dtype": "float64", "device": torch.cuda.get_device_name(0),
              "chunk_maps": per, "device_ms": device_ms, "device_runs_ms": device_runs,
              "device_and_copies_ms": copies_ms, "device_and_copies_runs_ms": copies_runs, "host_threads": THREADS,
              "host_maps_timed": m, "host_ms_timed": host_ms, "host_ms_scaled_to_maps": host_ms * N / m,
              "first_canvases_equal_bytes": bool(equal), "compared": k}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))
    if not equal:
        raise SystemExit("the canvases of the two paths differ")


if __name__ == "__main__":
    main()
