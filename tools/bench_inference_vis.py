"""Times the two pictures of run_inference.py for a KITTI-Eigen-sized set (no dataset needed): 697 generated disparity
maps of 256 x 832, the bone picture of disp / max(disp) and the rainbow picture of (1 / disp) / 10 for each.

    python tools/bench_inference_vis.py [--maps 697] [--out profiles/inference_vis_bench.json]

  kernels    scsfm_hip.visualise.colourise, twice, with the maps already on the device (one call per picture kind for all
             maps; median of the repetitions, timed with events after a warm-up call), and the same followed by the
             copies back to the host
  host       the reference's chain per image -- max, divide, matplotlib colour map (bone resampled to 10 000 entries,
             the rainbow of scsfm_hip.visualise's stops with 1000), float32, times 255, uint8 -- on 16 host threads
The first maps' pictures of the two paths are compared byte for byte.  Writes one JSON file.  Needs a HIP device and
matplotlib."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sc-sfmlearner-release_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from scsfm_hip import visualise  # noqa: E402

THREADS = 16
H, W = 256, 832


def host_maps():
    import matplotlib
    from matplotlib.colors import LinearSegmentedColormap
    return {"bone": matplotlib.colormaps["bone"].resampled(10000),
            "rainbow": LinearSegmentedColormap.from_list("opencv_rainbow", visualise._RAINBOW, 1000)}


def host_pictures(disp, cmaps):
    """One float32 [H, W] disparity -> the two uint8 [H, W, 4] pictures, as tensor2array and run_inference.py do."""
    with np.errstate(all="ignore"):
        a = (255 * cmaps["bone"](disp / float(disp.max())).astype(np.float32)).astype(np.uint8)
        b = (255 * cmaps["rainbow"]((1 / disp) / 10).astype(np.float32)).astype(np.uint8)
    return a, b


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "inference_vis_bench.json"))
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_inference_vis.py needs a HIP device")
    rng = np.random.default_rng(0)
    # sigmoid-like disparities in (0.01, 10.01), smooth in the image with noise on top
    ramp = np.linspace(0.0, 1.0, H, dtype=np.float32)[:, None] ** 2
    disp = np.stack([(0.01 + 10.0 * (0.02 + 0.3 * ramp * rng.random()) * (0.8 + 0.4 * rng.random((H, W), dtype=np.float32)))
                     .astype(np.float32) for _ in range(args.maps)])
    staged = torch.from_numpy(disp).cuda()

    both = lambda: visualise.disparity_and_depth_images(staged)
    kernels_ms, kernel_runs = median_ms(both, args.reps)
    with_copy_ms, copy_runs = median_ms(lambda: [p.cpu() for p in both()], args.reps)

    cmaps = host_maps()
    t0 = time.perf_counter()
    with ThreadPoolExecutor(THREADS) as pool:
        host = list(pool.map(lambda d: host_pictures(d, cmaps), disp))
    host_ms = (time.perf_counter() - t0) * 1e3

    k = min(8, args.maps)
    got = [p[:k].cpu().numpy() for p in both()]
    equal = all(np.array_equal(got[0][i], host[i][0]) and np.array_equal(got[1][i], host[i][1]) for i in range(k))
    result = {"maps": args.maps, "height": H, "width": W, "device": torch.cuda.get_device_name(0),
              "kernels_ms": kernels_ms, "kernels_runs_ms": kernel_runs, "kernels_and_copies_ms": with_copy_ms,
              "kernels_and_copies_runs_ms": copy_runs, "host_threads": THREADS, "host_ms": host_ms,
              "first_pictures_equal_bytes": bool(equal), "compared": k}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))
    if not equal:
        raise SystemExit("the pictures of the two paths differ")


if __name__ == "__main__":
    main()
