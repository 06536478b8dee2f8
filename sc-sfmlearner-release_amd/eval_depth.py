"""Evaluates depth predictions against ground truth -- the reference's eval_depth.py (same flags, same printout), with
the per-pixel work in HIP (scsfm_hip.depth_eval, libscsfm_eval.so).

    python eval_depth.py --dataset kitti --pred_depth results/predictions.npy --gt_depth kitti_depth_test/depth
    python eval_depth.py --dataset nyu --pred_depth results/predictions.npy --gt_depth nyu_test/depth.npy

KITTI's GT is the name-sorted ``*.npy`` files of a folder (ragged sizes), NYU's one [N, H, W] ``.npy``.  Depth
visualisation (--vis_dir / --img_dir) is not implemented.
"""
import argparse
import glob
import os
import sys

parser = argparse.ArgumentParser(description="NYUv2 Depth options")
parser.add_argument("--dataset", required=True, help="kitti or nyu", choices=['nyu', 'kitti'], type=str)
parser.add_argument("--pred_depth", required=True, help="depth predictions npy", type=str)
parser.add_argument("--gt_depth", required=True, help="gt depth nyu for nyu or folder for kitti", type=str)
parser.add_argument("--vis_dir", help="result directory for saving visualization (not implemented)", type=str)
parser.add_argument("--img_dir", help="image directory for reading image (not implemented)", type=str)
parser.add_argument("--ratio_name", help="names for saving ratios", type=str)


def load_gt(dataset, path):
    import numpy as np
    if dataset == 'nyu':
        return np.load(path)
    files = sorted(glob.glob(os.path.join(path, "*.npy")))
    if not files:
        raise SystemExit(f"eval_depth.py: no *.npy ground truth under {path}")
    return [np.load(f) for f in files]


def main(argv=None):
    args = parser.parse_args(argv)
    if args.vis_dir or args.img_dir:
        parser.error("--vis_dir / --img_dir (depth visualisation) are not implemented here; "
                     "evaluate without them")
    import numpy as np

    from scsfm_hip.depth_eval import evaluate_depth

    pred_depths = np.load(args.pred_depth)
    gt_depths = load_gt(args.dataset, args.gt_depth)
    print("==> Evaluating depth result...")
    res = evaluate_depth(gt_depths, pred_depths, args.dataset, eval_mono=True)
    lines = res.report_lines()
    print("\n".join(lines[:2]))
    if args.ratio_name:
        np.savetxt(args.ratio_name, res.ratios, fmt='%.4f')
    print("\n".join(lines[2:]))
    return res


if __name__ == "__main__":
    sys.exit(0 if main() is not None else 1)
