"""Compiles the validation kernels (sc-sfmlearner-release_amd/csrc_val/*.hip), unchanged, against the host simulator
(tests/hostsim/hip/hip_runtime.h) with g++ into tests/hostsim/_build_val/, and runs the C ABI of include/scsfm_val.h on
HOST pointers.  Test infrastructure only; never loaded by the product."""
from __future__ import annotations

import ctypes
import functools
import os

import numpy as np

import validation_errors_oracle as O
from hostsim import library
from scsfm_hip._lib import VAL_ABI_VERSION, VAL_HEADER, CLib

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(ROOT, "sc-sfmlearner-release_amd", "csrc_val")
HOSTSIM = os.path.join(HERE, "hostsim")
OUT = os.path.join(HOSTSIM, "_build_val")
LIB = os.path.join(OUT, "libscsfm_val_hostsim.so")

GUARD = 16                  # elements of guard band after every output
SENTINEL = {"metrics": -12345.5, "medians": -54321.5, "count": -77}


def build(force=False):
    return library.build("val", force, dep=os.path.abspath(__file__))


@functools.lru_cache(maxsize=1)
def lib():
    return CLib(build(), VAL_HEADER, VAL_ABI_VERSION, "scsfm_val_")


def _ptr(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def outputs(B):
    """The three output buffers, each pre-filled with its sentinel and followed by a guard band."""
    return dict(metrics=np.full(B * 6 + GUARD, SENTINEL["metrics"], np.float64),
                medians=np.full(B * 2 + GUARD, SENTINEL["medians"], np.float32),
                count=np.full(B + GUARD, SENTINEL["count"], np.int32))


def untouched(bufs, B=0):
    """True when everything past the first B rows of every output still holds its sentinel."""
    return all(bool((bufs[k][B * per:] == SENTINEL[k]).all()) for k, per in (("metrics", 6), ("medians", 2), ("count", 1)))


def raw(B, h, w, src, is_disp, H, W, gt, box, min_gt, max_depth, clamp_lo, ws, ws_bytes, bufs, null=()):
    """scsfm_val_depth_errors' status for exactly these arguments; ``null`` names pointers to pass as NULL."""
    p = {k: (None if k in null else _ptr(v)) for k, v in
         dict(src=src, gt=gt, ws=ws, metrics=bufs["metrics"], medians=bufs["medians"], count=bufs["count"]).items()}
    return lib()._fn["scsfm_val_depth_errors"](B, h, w, p["src"], is_disp, H, W, p["gt"], *box, min_gt, max_depth,
                                               clamp_lo, p["ws"], ws_bytes, p["metrics"], p["medians"], p["count"],
                                               None)


def depth_errors(gt, src, dataset, is_disp=False):
    """scsfm_hip.validation.depth_errors on the simulator -> dict(metrics[B,6], medians[B,2], count[B]).  The outputs
    start as sentinels, and the guard bands behind them must come back intact."""
    gt, src = np.ascontiguousarray(gt, np.float32), np.ascontiguousarray(src, np.float32)
    B, H, W = gt.shape
    h, w = src.shape[1:]
    y1, y2, x1, x2, cap = O.crop_and_cap(dataset, H, W)
    nbytes = lib().size("scsfm_val_workspace_bytes", B, H, W)
    assert nbytes > 0
    ws = np.full(nbytes + 64, 0xAB, np.uint8)
    bufs = outputs(B)
    rc = raw(B, h, w, src, int(is_disp), H, W, gt, (y1, y2, x1, x2), 0.1, float(cap), 1e-3, ws, nbytes, bufs)
    assert rc == 0, rc
    assert untouched(bufs, B) and (ws[nbytes:] == 0xAB).all()
    return dict(metrics=bufs["metrics"][:B * 6].reshape(B, 6).copy(), medians=bufs["medians"][:B * 2].reshape(B, 2).copy(),
                count=bufs["count"][:B].copy())
