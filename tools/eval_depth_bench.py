"""Times depth evaluation (scsfm_hip.depth_eval.evaluate_depth, libscsfm_eval.so) at full scale on one GPU:

  kitti  697 ragged GT maps of the four KITTI Eigen sizes (about 4 % valid, float32), float64 256x832 predictions
  nyu    654 dense 480x640 GT maps (float32), float64 256x320 predictions

and, per set: the wall time of evaluate_depth with device-resident inputs and from .npy files (load + evaluate, files
just written: page cache warm), the compulsory bytes (GT and predictions read once) against 8 TB/s, and the oracle's
per-image numpy loop on the host (tests/depth_eval_oracle.py) timed on the first --oracle-images images and scaled to
the set.  The maps are a seeded bank of 48 (KITTI) / 32 (NYU) distinct images repeated, which changes nothing in the
work per image.  For the per-kernel breakdown run it under rocprofv3 with --reps 2 --no-oracle --no-files:

    python tools/eval_depth_bench.py --out results/eval_bench.json
    rocprofv3 --kernel-trace --stats -d results/prof -o eval -- python tools/eval_depth_bench.py --reps 2 --no-oracle --no-files
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "sc-sfmlearner-release_amd"), os.path.join(ROOT, "tests")]

import _depth_eval_data as D  # noqa: E402
import depth_eval_oracle as O  # noqa: E402
from scsfm_hip.depth_eval import evaluate_depth  # noqa: E402

HBM = 8e12


def kitti_set(n=697, bank=48):
    gts, pred = D.kitti_set(bank, seed=31)
    idx = np.arange(n) % bank
    return [gts[i] for i in idx], pred[idx]


def nyu_set(n=654, bank=32):
    gts, pred = D.nyu_set(bank, seed=32)
    idx = np.arange(n) % bank
    return gts[idx], pred[idx]


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t)
    return ts


def run(name, gts, pred, args):
    out = {"images": len(pred), "pred": list(pred.shape[1:]), "pred_dtype": str(pred.dtype)}
    dev = torch.device("cuda")
    if isinstance(gts, list):
        d_gts = [torch.from_numpy(g).to(dev) for g in gts]
        gt_bytes = sum(g.nbytes for g in gts)
    else:
        d_gts = torch.from_numpy(gts).to(dev)
        gt_bytes = gts.nbytes
    d_pred = torch.from_numpy(pred).to(dev)
    res = evaluate_depth(d_gts, d_pred, name)
    out["valid_pixels"] = int(res.count.sum())
    out["gt_pixels"] = int(gt_bytes // 4)
    out["report"] = res.report_lines()
    ts = timed(lambda: evaluate_depth(d_gts, d_pred, name), args.reps)
    out["device_resident_s"] = {"min": min(ts), "median": float(np.median(ts)), "reps": len(ts)}
    out["compulsory_bytes"] = int(gt_bytes + pred.nbytes)
    out["compulsory_bytes_over_min_time_TBps"] = out["compulsory_bytes"] / min(ts) / 1e12
    out["share_of_8TBps"] = out["compulsory_bytes"] / min(ts) / HBM
    if not args.no_files:
        with tempfile.TemporaryDirectory() as tmp:
            np.save(os.path.join(tmp, "pred.npy"), pred)
            if name == "kitti":
                os.mkdir(os.path.join(tmp, "gt"))
                for i, g in enumerate(gts):
                    np.save(os.path.join(tmp, "gt", f"{i:06d}.npy"), g)
            else:
                np.save(os.path.join(tmp, "gt.npy"), gts)

            def from_files():
                p = np.load(os.path.join(tmp, "pred.npy"))
                if name == "kitti":
                    files = sorted(os.listdir(os.path.join(tmp, "gt")))
                    g = [np.load(os.path.join(tmp, "gt", f)) for f in files]
                else:
                    g = np.load(os.path.join(tmp, "gt.npy"))
                evaluate_depth(g, p, name)

            ts = timed(from_files, max(1, args.reps // 2))
            out["from_npy_files_s"] = {"min": min(ts), "median": float(np.median(ts)), "reps": len(ts)}
    if not args.no_oracle:
        k = args.oracle_images
        t = time.perf_counter()
        O.evaluate(list(gts[:k]), pred[:k], name)
        dt = time.perf_counter() - t
        out["oracle_numpy_loop"] = {"images_timed": k, "s_per_image": dt / k, "scaled_to_set_s": dt / k * len(pred)}
        out["speedup_vs_oracle_loop"] = dt / k * len(pred) / out["device_resident_s"]["min"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", default="kitti,nyu")
    ap.add_argument("--reps", type=int, default=6)
    ap.add_argument("--oracle-images", type=int, default=12)
    ap.add_argument("--no-oracle", action="store_true")
    ap.add_argument("--no-files", action="store_true")
    ap.add_argument("--out")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("eval_depth_bench.py needs a HIP device")
    result = {"device": torch.cuda.get_device_name(0)}
    for name in args.sets.split(","):
        gts, pred = kitti_set() if name == "kitti" else nyu_set()
        result[name] = run(name, gts, pred, args)
        print(json.dumps({name: {k: v for k, v in result[name].items() if k != "report"}}), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
