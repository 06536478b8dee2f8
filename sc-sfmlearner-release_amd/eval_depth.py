"""Evaluates depth predictions against ground truth -- the reference's eval_depth.py (same flags, same printout), with
the per-pixel work in HIP (scsfm_hip.depth_eval, libscsfm_eval.so).

    python eval_depth.py --dataset kitti --pred_depth results/predictions.npy --gt_depth kitti_depth_test/depth
    python eval_depth.py --dataset nyu --pred_depth results/predictions.npy --gt_depth nyu_test/depth.npy

    python eval_depth.py --dataset nyu ... --vis_dir results --img_dir nyu_test/color

KITTI's GT is the name-sorted ``*.npy`` files of a folder (ragged sizes), NYU's one [N, H, W] ``.npy``.  With --vis_dir
(which needs --img_dir) one picture per evaluated prediction is written to ``<vis_dir>/vis_depth/%04d.png`` after the
table: the photograph beside the magma picture of the resized, median-scaled prediction and, on NYU, beside the ground
truth's picture in the same colour scale (scsfm_hip.depth_vis, libscsfm_dvis.so).  Photographs are the name-sorted
``*.png`` files of --img_dir, read and written with Pillow.
"""
import argparse
import glob
import os
import sys

parser = argparse.ArgumentParser(description="NYUv2 Depth options")
parser.add_argument("--dataset", required=True, help="kitti or nyu", choices=['nyu', 'kitti'], type=str)
parser.add_argument("--pred_depth", required=True, help="depth predictions npy", type=str)
parser.add_argument("--gt_depth", required=True, help="gt depth nyu for nyu or folder for kitti", type=str)
parser.add_argument("--vis_dir", help="result directory for saving visualization", type=str)
parser.add_argument("--img_dir", help="image directory for reading image", type=str)
parser.add_argument("--ratio_name", help="names for saving ratios", type=str)


def load_gt(dataset, path):
    import numpy as np
    if dataset == 'nyu':
        return np.load(path)
    files = sorted(glob.glob(os.path.join(path, "*.npy")))
    if not files:
        raise SystemExit(f"eval_depth.py: no *.npy ground truth under {path}")
    return [np.load(f) for f in files]


# pixels of ground truth per visualisation chunk: bounds the scaled predictions, the workspace and the canvases on the
# device (about 30 bytes per pixel with float64 maps)
VIS_CHUNK_PIXELS = 1 << 24
DEVICE = "cuda"
PNG_THREADS = 8  # host threads that decode photographs and encode pictures (never sized by the machine's CPU count)


def read_photo(path):
    """uint8 [H, W, 3] RGB, as cv2.imread(path, 1) + BGR->RGB gives for 8-bit RGB and grey files."""
    import numpy as np
    from PIL import Image
    with Image.open(path) as im:
        return np.array(im.convert('RGB'))


def write_picture(path, rgb):
    from PIL import Image
    Image.fromarray(rgb, 'RGB').save(path)


def visualise(args, res, gt_depths, pred_depths):
    """Writes <vis_dir>/vis_depth/%04d.png for every evaluated prediction; returns the files' paths."""
    from concurrent.futures import ThreadPoolExecutor

    import torch

    from scsfm_hip import depth_vis

    sizes = depth_vis.picture_sizes(res, gt_depths)
    image_paths = sorted(glob.glob(os.path.join(args.img_dir, "*.png")))
    if len(image_paths) < len(sizes):
        raise SystemExit(f"eval_depth.py: {len(sizes)} predictions to visualise but only {len(image_paths)} *.png "
                         f"under {args.img_dir}")
    if len(sizes) < len(res.evaluated):
        print(f"eval_depth.py: {len(res.evaluated) - len(sizes)} predictions were skipped (mean -1): picture k shows "
              f"the k-th evaluated prediction beside photograph k, as in the reference", file=sys.stderr)
    save_folder = os.path.join(args.vis_dir, 'vis_depth')
    os.makedirs(save_folder, exist_ok=True)
    written, pending = [], []
    with ThreadPoolExecutor(max_workers=PNG_THREADS) as pool:
        k0 = 0
        while k0 < len(sizes):
            k1, pixels = k0, 0
            while k1 < len(sizes) and (k1 == k0 or pixels + sizes[k1][0] * sizes[k1][1] <= VIS_CHUNK_PIXELS):
                pixels += sizes[k1][0] * sizes[k1][1]
                k1 += 1
            photos = list(pool.map(read_photo, image_paths[k0:k1]))
            for k, img in zip(range(k0, k1), photos):
                if img.shape[:2] != sizes[k]:
                    raise SystemExit(f"eval_depth.py: {image_paths[k]} is {img.shape[0]} x {img.shape[1]} but the depth "
                                     f"map of picture {k} is {sizes[k][0]} x {sizes[k][1]}")
            canvases = depth_vis.composites(res, pred_depths, gt_depths, args.dataset,
                                            [torch.from_numpy(p).to(DEVICE) for p in photos], first=k0)
            for k, c in zip(range(k0, k1), canvases):
                path = os.path.join(save_folder, "{:04}.png".format(k))
                pending.append(pool.submit(write_picture, path, c.cpu().numpy()))
                written.append(path)
            k0 = k1
        for f in pending:
            f.result()
    return written


def main(argv=None):
    args = parser.parse_args(argv)
    if args.vis_dir and not args.img_dir:
        parser.error("--vis_dir needs --img_dir (the folder of the photographs)")
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
    if args.vis_dir:
        visualise(args, res, gt_depths, pred_depths)
    return res


if __name__ == "__main__":
    sys.exit(0 if main() is not None else 1)
