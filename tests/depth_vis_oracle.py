"""An independent numpy restatement of the reference's depth visualisation (eval_depth.py: what evaluate_depth returns,
depth_visualizer, depth_pair_visualizer and the canvases of main), written out operation by operation so that every
rounding is visible.  It is the yardstick of libscsfm_dvis.so (include/scsfm_dvis.h) and of scsfm_hip.depth_vis;
tests/test_depth_vis_reference.py holds it to the reference's own functions under the installed numpy and matplotlib.

  - ``scaled_prediction``: 1 / (resize_linear(1 / (pred + 1e-6)) + 1e-6) in the prediction's precision, times the ratio
    in the promoted precision (tests/depth_eval_oracle.py: resize_linear is OpenCV's INTER_LINEAR);
  - ``percentile95``: np.percentile(a, 95) from a full sort: the virtual index, its floor and the weight in the array's
    own precision, then numpy's _lerp with its two branches;
  - ``colourise``: matplotlib's Normalize (in-place -= and /= with float64 scalars: computed in double, rounded back after
    each step), the multiplication by 256 and Colormap.__call__'s under / over / bad rules on a 256 x 3 byte table.
"""
from __future__ import annotations

import warnings

import numpy as np

import depth_eval_oracle as E


def scaled_prediction(pred, ratio, height, width, rdt):
    """pred [h, w] -> [height, width] of dtype rdt: the reference's ``pred_depth * ratio``."""
    with np.errstate(all="ignore"):
        inv = 1 / (pred + 1e-6)
        depth = 1 / (E.resize_linear(inv, width, height) + 1e-6)
        assert depth.dtype == pred.dtype
        return depth.astype(rdt) * np.dtype(rdt).type(ratio)


def percentile_index(n, dtype):
    T = np.dtype(dtype).type
    q = T(95) / T(100)
    vi = T(n - 1) * q
    lo = int(np.floor(vi))
    hi = min(lo + 1, n - 1)
    return lo, hi, T(vi - T(lo))


def percentile95(a):
    a = np.asarray(a)
    T = a.dtype.type
    if np.isnan(a).any():
        return T(np.nan)
    s = np.sort(a.ravel())
    lo, hi, t = percentile_index(s.size, a.dtype)
    with np.errstate(all="ignore"):
        x, y = s[lo], s[hi]
        d = T(y - x)
        return T(x + T(d * t)) if t < 0.5 else T(y - T(d * T(T(1) - t)))


def inverse(x):
    with np.errstate(all="ignore"):
        inv = 1 / (x + 1e-6)
    assert inv.dtype == x.dtype
    return inv


def depth_range(x):
    """(vmin, vmax) of a map, numpy scalars of its dtype; both NaN when the map's inverse holds one."""
    inv = inverse(np.asarray(x))
    T = inv.dtype.type
    if np.isnan(inv).any():
        return T(np.nan), T(np.nan)
    return inv.min(), percentile95(inv)


def colourise(x, vmin, vmax, table):
    """uint8 [H, W, 3]: the magma picture of 1 / (x + 1e-6) in the range (vmin, vmax)."""
    inv = inverse(np.asarray(x))
    T = inv.dtype.type
    vmin, vmax = float(vmin), float(vmax)
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        if vmin == vmax:
            v = np.zeros_like(inv)
        else:
            v = (inv.astype(np.float64) - vmin).astype(T)
            v = (v.astype(np.float64) / (vmax - vmin)).astype(T)
        xa = v * T(256)
        idx = np.where(xa >= 256, 255, np.where(xa < 0, 0, np.nan_to_num(xa, nan=0.0))).astype(np.int64)
        out = np.asarray(table)[np.clip(idx, 0, 255)]
        out[np.isnan(xa)] = 0
    return out


def depth_picture(x, table):
    return colourise(x, *depth_range(x), table)


def pair_pictures(pred, gt, table):
    vmin, vmax = depth_range(gt)
    return colourise(pred, vmin, vmax, table), colourise(gt, vmin, vmax, table)


def evaluated(pred_depths):
    return [i for i, p in enumerate(pred_depths) if np.asarray(p).mean() != -1]


def composites(gt_depths, pred_depths, ratios, dataset, photos, table):
    """The canvases of the reference's main: ``ratios[i]`` is image i's median ratio (any value for a skipped one);
    picture k pairs the k-th evaluated prediction with photograph k and, on NYU, ground truth k."""
    rdt = np.result_type(np.asarray(gt_depths[0]).dtype, np.asarray(pred_depths).dtype)
    out = []
    for k, i in enumerate(evaluated(pred_depths)):
        H, W = np.asarray(gt_depths[i]).shape
        scaled = scaled_prediction(np.asarray(pred_depths[i]), ratios[i], H, W, rdt)
        img = np.asarray(photos[k])
        h, w, _ = img.shape
        if dataset == "nyu":
            cat = np.zeros((h, 3 * w, 3), np.uint8)
            cat[:, :w] = img
            cat[:, w:2 * w], cat[:, 2 * w:] = pair_pictures(scaled, np.asarray(gt_depths[k]), table)
        else:
            cat = np.zeros((2 * h, w, 3), np.uint8)
            cat[:h] = img
            cat[h:] = depth_picture(scaled, table)
        out.append(cat)
    return out
