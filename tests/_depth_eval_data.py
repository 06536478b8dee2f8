"""Seeded synthetic evaluation sets shaped like KITTI Eigen (ragged, sparse GT, cropped) and NYUv2 (dense GT) for the
depth-evaluation tests.  Depth fields are the smooth random fields of scsfm_hip.synth; the GT is quantised to 1/256 m as
KITTI's 16-bit PNGs are, so that ties at the median are common."""
from __future__ import annotations

import numpy as np
import torch

from scsfm_hip import synth

KITTI_SIZES = ((375, 1242), (370, 1224), (374, 1238), (376, 1241))


def _field(rng, n, h, w, coarse=(5, 9)):
    return synth._lowpass(rng, (n, 1, h, w), coarse)[:, 0].numpy().astype(np.float64)


def kitti_set(n, seed=0, sizes=KITTI_SIZES, pred_hw=(256, 832), density=0.04, pred_dtype=np.float64,
              gt_dtype=np.float32):
    """n ragged GT maps cycling through ``sizes`` (about ``density`` valid, some beyond 80 m) and [n, h, w] predictions
    whose scale is unknown (median scaling is the point)."""
    rng = np.random.default_rng(seed)
    gts = []
    for i in range(n):
        H, W = sizes[i % len(sizes)]
        d = 1.0 + 95.0 * _field(rng, 1, H, W)[0] ** 1.5
        d = np.round(d * 256) / 256
        d[rng.random((H, W)) >= density] = 0.0
        gts.append(d.astype(gt_dtype))
    h, w = pred_hw
    pred = (0.02 + 3.0 * _field(rng, n, h, w) ** 1.5) * rng.uniform(0.5, 2.0, (n, 1, 1))
    return gts, pred.astype(pred_dtype)


def nyu_set(n, seed=0, gt_hw=(480, 640), pred_hw=(256, 320), pred_dtype=np.float64, gt_dtype=np.float32):
    """[n, H, W] dense GT (about 80 % inside (1e-3, 10)) and [n, h, w] predictions."""
    rng = np.random.default_rng(seed)
    H, W = gt_hw
    d = 0.5 + 11.0 * _field(rng, n, H, W)
    d = np.round(d * 1000) / 1000
    d[rng.random((n, H, W)) < 0.05] = 0.0
    h, w = pred_hw
    pred = (0.1 + 2.0 * _field(rng, n, h, w)) * rng.uniform(0.5, 2.0, (n, 1, 1))
    return d.astype(gt_dtype), pred.astype(pred_dtype)


def to_torch(x):
    return torch.from_numpy(np.ascontiguousarray(x))
