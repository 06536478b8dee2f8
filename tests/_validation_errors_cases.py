"""Inputs of the validation-error tests (host simulator and GPU): the smallest shapes at which the pieces of
libscsfm_val.so can go wrong, and the planted edge cases.  Each case is built once and its arrays are read-only."""
from __future__ import annotations

import functools

import numpy as np

import validation_errors_oracle as O

F32 = np.float32


def _freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def _disp(rng, B, h, w):
    """A disparity like the network's sigmoid output: 1 / disp spans 0.6 .. 125, past both depth caps."""
    return rng.uniform(0.008, 1.6, (B, h, w)).astype(F32)


def _parity(gt, dataset, odd):
    """Zeroes one valid pixel if the valid count's parity is not the wanted one."""
    y1, y2, x1, x2, cap = O.crop_and_cap(dataset, *gt.shape)
    valid = np.zeros(gt.shape, bool)
    valid[y1:y2, x1:x2] = (gt[y1:y2, x1:x2] > O.MIN_GT) & (gt[y1:y2, x1:x2] < cap)
    if int(valid.sum()) % 2 != int(odd):
        r, c = np.argwhere(valid)[len(np.argwhere(valid)) // 3]
        gt[r, c] = 0
    return gt


@functools.lru_cache(maxsize=None)
def case_a():
    """kitti, disparity 16x52 against GT 37x124 (a non-integer scale; the crop box is rows 15:36, columns 4:119), B=3:
    (a) an odd valid count, (b) an even one, (c) a GT in multiples of 1/256 on a few levels with about 70 % zeros, like
    KITTI's projected lidar, so that the middle ranks are ties."""
    rng = np.random.default_rng(11)
    gt = rng.uniform(0.05, 90.0, (3, 37, 124)).astype(F32)  # some below 0.1, some beyond 80
    _parity(gt[0], "kitti", odd=True)
    _parity(gt[1], "kitti", odd=False)
    levels = (np.arange(1, 15) * 1391 % 20000 + 300).astype(F32) / F32(256)
    gt[2] = levels[rng.integers(0, len(levels), (37, 124))]
    gt[2][rng.random((37, 124)) < 0.7] = 0
    return _freeze(gt, _disp(rng, 3, 16, 52)) + ("kitti",)


@functools.lru_cache(maxsize=None)
def case_b():
    """nyu, 48x64 for both (no resize; the crop box is rows 4:47, columns 4:60), B=2."""
    rng = np.random.default_rng(12)
    gt = rng.uniform(0.05, 11.0, (2, 48, 64)).astype(F32)
    return _freeze(gt, _disp(rng, 2, 48, 64)) + ("nyu",)


@functools.lru_cache(maxsize=None)
def case_c():
    """nyu, 192x640, one image, every pixel of the crop box valid: 95,030 pairs, so the counters, the scan and the
    histogram bins pass 16 bits; few distinct GT values, so that single bins do."""
    rng = np.random.default_rng(13)
    gt = (rng.integers(1, 4, (1, 192, 640)) * F32(2.5)).astype(F32)
    return _freeze(gt, _disp(rng, 1, 192, 640)) + ("nyu",)


CASES = {"A": case_a, "B": case_b, "C": case_c}


@functools.lru_cache(maxsize=None)
def expected(name, is_disp=True):
    """The oracle's result of a case (computed once)."""
    gt, src, dataset = CASES[name]()
    return O.depth_errors(gt, src, dataset, is_disp)


def edge(kind):
    """-> (gt[3, 37, 124], src[3, 37, 124] depth, 'kitti'): case A's ground truth with image 1 doctored."""
    gt, _, dataset = case_a()
    gt = gt.copy()
    rng = np.random.default_rng(14)
    src = rng.uniform(0.5, 70.0, gt.shape).astype(F32)
    y1, y2, x1, x2, _ = O.crop_and_cap(dataset, 37, 124)
    if kind == "empty":
        gt[1] = 0
        gt[1, :y1] = 5  # valid depths, all outside the crop box
    elif kind == "one_pixel":
        gt[1] = 0
        gt[1, y1 + 3, x1 + 7] = 12.5
    elif kind == "all_equal":
        gt[1, y1:y2, x1:x2] = 7.25
    elif kind == "nan_pred":
        src[1, y1 + 2, x1 + 2] = np.nan
        gt[1, y1 + 2, x1 + 2] = 9.0
    elif kind == "nan_outside":  # a NaN prediction where the GT is invalid changes nothing
        src[1, 0, 0] = np.nan
        src[1, y1 + 2, x1 + 2] = np.nan
        gt[1, y1 + 2, x1 + 2] = 0
    elif kind == "nan_gt":
        gt[1, y1 + 2, x1 + 2] = np.nan
        gt[1, y1 + 4, x1 + 9] = np.inf
    elif kind == "clamp":
        src[1, y1:y2:2, x1:x2:3] = 2e-4   # below clamp_lo
        src[1, y1:y2:3, x1:x2:2] = 300.0  # beyond the cap
        src[1, y1 + 1, x1 + 1] = -4.0
        src[1, y1 + 1, x1 + 2] = np.inf
        src[1, y1 + 1, x1 + 3] = -np.inf
    else:
        raise KeyError(kind)
    return gt, src, dataset


EDGES = ("empty", "one_pixel", "all_equal", "nan_pred", "nan_outside", "nan_gt", "clamp")


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


def check(got, want, torch_medians=None):
    """``got``: dict(metrics[B,6], medians[B,2], count[B]) of the library; ``want``: the oracle's list.  Counts and the
    thresholds' counts exact, medians bit for bit, the three means to 1e-12 of the float64 sums."""
    B = len(want)
    assert got["metrics"].shape == (B, 6) and got["medians"].shape == (B, 2) and got["count"].shape == (B,)
    assert got["metrics"].dtype == np.float64 and got["medians"].dtype == F32 and got["count"].dtype == np.int32
    for i, w in enumerate(want):
        n = w["n"]
        assert got["count"][i] == n, (i, got["count"][i], n)
        assert same_bits(got["medians"][i], np.array([w["med_gt"], w["med_pred"]], F32)), (i, got["medians"][i], w)
        m = got["metrics"][i]
        if np.isnan(w["metrics"]).all():
            assert np.isnan(m).all(), (i, m)
            continue
        assert np.array_equal(np.rint(m[3:] * n).astype(np.int64), w["hits"]) and \
            np.array_equal(m[3:], w["hits"] / n), (i, m[3:] * n, w["hits"])
        np.testing.assert_allclose(m[:3] * n, w["sums"], rtol=1e-12, atol=0)
        np.testing.assert_allclose(m[:3], w["metrics"][:3], rtol=1e-12, atol=0)
