"""What train.py --log-output computes around the networks, written out in numpy: the float pictures the reference's
tensor2array returns, their bytes, the de-normalised input and the target disparity.  Independent of
scsfm_hip.validation_log's kernels (which the tests judge with it); the tables are arguments, so that the goldens' own
tables (recorded from the reference) can be used.  tests/test_validation_log_reference.py ties it to the goldens and to
the live reference.

    xa = (x / d) * N in float32;  NaN -> (0, 0, 0, 0);  xa < 0 -> table[0];  xa >= N -> table[N - 1];  else table[int(xa)]
    byte = uint8(min(max(float32(255) * v, 0), 255)), NaN -> 0
"""
import numpy as np


def to_bytes(v):
    with np.errstate(all="ignore"):
        t = np.float32(255) * np.asarray(v, dtype=np.float32)
        t = np.where(t > 0, t, np.float32(0))  # (a NaN fails the comparison)
        return np.where(t < 255, t, np.float32(255)).astype(np.uint8)


def map_picture(one, table, max_value=None):
    """One float32 [H, W] map -> float32 [4, H, W]."""
    one = np.asarray(one, dtype=np.float32)
    n = len(table)
    with np.errstate(all="ignore"):
        d = one.max() if max_value is None else np.float32(max_value)
        xa = ((one / np.float32(d)).astype(np.float32) * np.float32(n)).astype(np.float32)
        idx = np.trunc(np.where(np.isfinite(xa), xa, 0)).astype(np.int64)
        idx = np.where(xa < 0, 0, idx)
        idx = np.where(xa >= n, n - 1, idx)
    out = np.asarray(table, dtype=np.float32)[np.clip(idx, 0, n - 1)].copy()
    out[np.isnan(xa)] = 0
    return np.ascontiguousarray(out.transpose(2, 0, 1))


def map_pictures(maps, table, max_value=None):
    """float32 [N, H, W] -> float32 [N, 4, H, W], every image on its own."""
    return np.stack([map_picture(m, table, max_value) for m in np.asarray(maps, dtype=np.float32)])


def map_bytes(maps, table, max_value=None):
    """float32 [N, H, W] -> uint8 [N, H, W, 4]."""
    return np.ascontiguousarray(to_bytes(map_pictures(maps, table, max_value)).transpose(0, 2, 3, 1))


def input_pictures(batch):
    """float32 [N, 3, H, W] -> float32 [N, 3, H, W]: the multiply rounded, then the add."""
    scaled = (np.asarray(batch, dtype=np.float32) * np.float32(0.225)).astype(np.float32)
    return (np.float32(0.45) + scaled).astype(np.float32)


def input_bytes(batch):
    """float32 [N, 3, H, W] -> uint8 [N, H, W, 3]."""
    return np.ascontiguousarray(to_bytes(input_pictures(batch)).transpose(0, 2, 3, 1))


def target_disparity(depth):
    """float32 [...] -> float32 [...]: 1 / depth with 1000 for every 0, clamped to [0, 10]; a NaN stays."""
    depth = np.asarray(depth, dtype=np.float32)
    with np.errstate(all="ignore"):
        r = (np.float32(1) / np.where(depth == 0, np.float32(1000), depth)).astype(np.float32)
        r = np.where(r < 0, np.float32(0), r)
        return np.where(r > 10, np.float32(10), r).astype(np.float32)
