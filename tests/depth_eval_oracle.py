"""An independent numpy restatement of the reference's monocular depth evaluation (eval_depth.py:
DepthEvalEigen.evaluate_depth + compute_depth_errors with eval_mono=True), one image at a time on the host.

It is the yardstick of libscsfm_eval.so (include/scsfm_eval.h) and of scsfm_hip.depth_eval:
  - ``resize_linear`` writes out OpenCV's INTER_LINEAR on its generic path: source coordinate (d + 0.5) * scale - 0.5
    with scale = 1 / (dst / src) in double, rounded to float32 and floored; below 0 -> index 0, weight 0; at or past
    src - 1 -> the last index, weight 0; float32 weights; rows first, then the two rows, in the input's precision;
  - medians, logs and every element-wise operation are numpy's own on the reference's dtypes (numpy 2 promotion);
  - the eight sums are taken in float64 (the kernels' contract; the reference sums in the promoted dtype).
An empty mask gives NaN metrics and a NaN ratio, as np.median of an empty array does in the reference.
"""
from __future__ import annotations

import warnings

import numpy as np

COLUMNS = ("abs_rel", "sq_rel", "rmse", "rmse_log", "log10", "a1", "a2", "a3")
DATASET_COLUMNS = {"kitti": ("abs_rel", "sq_rel", "rmse", "rmse_log", "a1", "a2", "a3"),
                   "nyu": ("abs_rel", "log10", "rmse", "a1", "a2", "a3")}
MAX_DEPTH = {"kitti": 80.0, "nyu": 10.0}
MIN_DEPTH = 1e-3


def _axis(dst, src):
    scale = 1.0 / (dst / src)
    f = ((np.arange(dst, dtype=np.float64) + 0.5) * scale - 0.5).astype(np.float32)
    i0 = np.floor(f).astype(np.int64)
    f = f - i0.astype(np.float32)
    lo = i0 < 0
    f[lo], i0[lo] = 0, 0
    hi = i0 >= src - 1
    f[hi], i0[hi] = 0, src - 1
    i1 = np.minimum(i0 + 1, src - 1)
    return i0, i1, np.float32(1) - f, f


def resize_linear(src, width, height):
    """cv2.resize(src, (width, height)) with INTER_LINEAR for a 2-D float32 / float64 array (see the module doc)."""
    src = np.asarray(src)
    dt = src.dtype
    h, w = src.shape
    x0, x1, ax0, ax1 = _axis(width, w)
    y0, y1, by0, by1 = _axis(height, h)
    ax0, ax1 = ax0.astype(dt), ax1.astype(dt)
    rows = src[:, x0] * ax0 + src[:, x1] * ax1  # every source row resized horizontally
    return rows[y0] * by0.astype(dt)[:, None] + rows[y1] * by1.astype(dt)[:, None]


def kitti_crop(H, W):
    return np.array([0.40810811 * H, 0.99189189 * H, 0.03594771 * W, 0.96405229 * W]).astype(np.int32)


def valid_pairs(gt, pred, dataset, min_depth=MIN_DEPTH, max_depth=None):
    """(gt[mask], resized pred[mask]) of one image, the reference's steps 1-2."""
    max_depth = MAX_DEPTH[dataset] if max_depth is None else max_depth
    H, W = gt.shape
    inv = 1 / (pred + 1e-6)
    pred_depth = 1 / (resize_linear(inv, W, H) + 1e-6)
    mask = np.logical_and(gt > min_depth, gt < max_depth)
    if dataset == "kitti":
        c = kitti_crop(H, W)
        crop = np.zeros(mask.shape, bool)
        crop[c[0]:c[1], c[2]:c[3]] = True
        mask &= crop
    return gt[mask], pred_depth[mask]


def errors(gt, pred):
    """The eight error terms of compute_depth_errors (COLUMNS order), element-wise in numpy's dtypes, sums in float64."""
    n = gt.size
    with np.errstate(all="ignore"):
        thresh = np.maximum(gt / pred, pred / gt)
        s = lambda x: np.sum(np.asarray(x, np.float64)) / n  # noqa: E731
        return np.array([s(np.abs(gt - pred) / gt), s(((gt - pred) ** 2) / gt), np.sqrt(s((gt - pred) ** 2)),
                         np.sqrt(s((np.log(gt) - np.log(pred)) ** 2)), s(np.abs(np.log10(gt) - np.log10(pred))),
                         s(thresh < 1.25), s(thresh < 1.25 ** 2), s(thresh < 1.25 ** 3)])


def evaluate_image(gt, pred, dataset, min_depth=MIN_DEPTH, max_depth=None):
    """-> dict(metrics[8], ratio, med_gt, med_pred, count, flag) of one image."""
    max_depth = MAX_DEPTH[dataset] if max_depth is None else max_depth
    nan = dict(metrics=np.full(8, np.nan), ratio=np.nan, med_gt=np.nan, med_pred=np.nan)
    if pred.mean() == -1:
        return dict(nan, count=0, flag=0)
    vg, vp = valid_pairs(gt, pred, dataset, min_depth, max_depth)
    if vg.size == 0:
        return dict(nan, count=0, flag=1)
    mg, mp = np.median(vg), np.median(vp)
    ratio = mg / mp
    vp = (vp * ratio).astype(vp.dtype)  # (the reference's in-place *=)
    vp[vp < min_depth] = min_depth
    vp[vp > max_depth] = max_depth
    return dict(metrics=errors(vg, vp), ratio=ratio, med_gt=mg, med_pred=mp, count=vg.size, flag=1)


def evaluate(gt_depths, pred_depths, dataset, min_depth=MIN_DEPTH, max_depth=None):
    """The whole set: per-image arrays, the mean in the dataset's column order, the ratio statistics."""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        per = [evaluate_image(np.asarray(g), np.asarray(p), dataset, min_depth, max_depth)
               for g, p in zip(gt_depths, pred_depths)]
        out = {k: np.array([d[k] for d in per]) for k in ("metrics", "ratio", "med_gt", "med_pred", "count", "flag")}
        ev = out["flag"] == 1
        cols = [COLUMNS.index(c) for c in DATASET_COLUMNS[dataset]]
        out["mean"] = out["metrics"][ev][:, cols].mean(0)
        rdt = np.result_type(np.asarray(gt_depths[0]).dtype, np.asarray(pred_depths).dtype)
        out["ratios"] = out["ratio"][ev].astype(rdt)
        out["ratio_stats"] = ratio_stats(out["ratios"])
    return out


def ratio_stats(ratios):
    """(median, std(ratios / median), mean, std) as the reference prints them."""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        med = np.median(ratios)
        return med, np.std(ratios / med), np.mean(ratios), np.std(ratios)


def report_lines(dataset, mean, stats):
    """The reference's printout after its progress bar (stdout), line by line."""
    med, std_rel, mean_r, std_r = stats
    cols = DATASET_COLUMNS[dataset]
    return [" Scaling ratios | med: {:0.3f} | std: {:0.3f}".format(med, std_rel),
            " Scaling ratios | mean: {:0.3f} +- std: {:0.3f}".format(mean_r, std_r),
            "",
            "  " + ("{:>8} | " * len(cols)).format(*cols),
            ("&{: 8.3f}  " * len(cols)).format(*np.asarray(mean).tolist()) + "\\\\"]
