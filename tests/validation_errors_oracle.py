"""numpy restatement of training's ground-truth validation metrics: validate_with_gt's 1 / disp and nearest resize and
compute_errors' per-image mask, clamp, lower-median scaling and six terms.  Written for the tests of libscsfm_val.so as
their independent comparand: every element-wise step is an fp32 numpy operation (IEEE, hence the very roundings of the
tensor operations), the medians are elements of a sorted copy, and the three sums are float64.
tests/test_validation_errors_reference.py pins it to the reference's compute_errors and to the committed goldens."""
from __future__ import annotations

import numpy as np

F32 = np.float32
MIN_GT, CLAMP_LO = F32(0.1), F32(1e-3)


def crop_and_cap(dataset, h, w):
    if dataset == "kitti":
        return int(0.40810811 * h), int(0.99189189 * h), int(0.03594771 * w), int(0.96405229 * w), F32(80)
    if dataset == "nyu":
        return int(0.09375 * h), int(0.98125 * h), int(0.0640625 * w), int(0.9390625 * w), F32(10)
    raise ValueError(dataset)


def nearest_index(out, inn):
    """F.interpolate(mode='nearest'): the source index of every destination index, with the scale in fp32."""
    scale = F32(inn) / F32(out)
    return np.minimum(np.floor(np.arange(out, dtype=F32) * scale).astype(np.int64), inn - 1)


def resize_nearest(img, H, W):
    return img[nearest_index(H, img.shape[0])][:, nearest_index(W, img.shape[1])]


def lower_median(x):
    """torch.median: NaN for nothing and for anything with a NaN in it, else the element of rank (n - 1) // 2."""
    if x.size == 0 or np.isnan(x).any():
        return F32(np.nan)
    return np.sort(x)[(x.size - 1) // 2]


def image_errors(gt, pred, dataset):
    """One image, ``pred`` already a depth at the ground truth's size -> dict(n, med_gt, med_pred, sums[3] float64,
    hits[3] int, metrics[6] float64)."""
    gt, pred = np.asarray(gt, F32), np.asarray(pred, F32)
    H, W = gt.shape
    y1, y2, x1, x2, cap = crop_and_cap(dataset, H, W)
    box = np.zeros((H, W), bool)
    box[y1:y2, x1:x2] = True
    with np.errstate(all="ignore"):
        valid = (gt > MIN_GT) & (gt < cap) & box
        g = gt[valid]
        p = pred[valid]
        p = np.where(np.isnan(p), p, np.minimum(np.maximum(p, CLAMP_LO), cap)).astype(F32)
        n = int(g.size)
        mg, mp = lower_median(g), lower_median(p)
        out = dict(n=n, med_gt=mg, med_pred=mp)
        if n == 0 or np.isnan(mp):
            out.update(sums=np.full(3, np.nan), hits=np.zeros(3, np.int64), metrics=np.full(6, np.nan))
            return out
        p = (p * mg) / mp
        assert p.dtype == F32
        d = g - p
        e = np.abs(d)
        t = np.maximum(g / p, p / g)
        terms = (e, e / g, (d * d) / g)
        assert all(x.dtype == F32 for x in terms) and t.dtype == F32
        sums = np.array([np.sum(x, dtype=np.float64) for x in terms])
        hits = np.array([int((t < F32(1.25)).sum()), int((t < F32(1.5625)).sum()), int((t < F32(1.953125)).sum())])
    out.update(sums=sums, hits=hits, metrics=np.concatenate([sums / n, hits / n]))
    return out


def depth_errors(gt, src, dataset, is_disp=False):
    """A batch: gt[B, H, W], src[B, h, w] (a depth, or a disparity with ``is_disp``) -> a list of image_errors."""
    out = []
    for g, s in zip(np.asarray(gt, F32), np.asarray(src, F32)):
        with np.errstate(all="ignore"):
            d = (F32(1) / s).astype(F32) if is_disp else s
        if d.shape != g.shape:
            d = resize_nearest(d, *g.shape)
        out.append(image_errors(g, d, dataset))
    return out


def batch_mean(images):
    """compute_errors' return value: the six sums over the batch divided by the batch size."""
    return (np.sum([im["metrics"] for im in images], axis=0) / len(images)).tolist()
