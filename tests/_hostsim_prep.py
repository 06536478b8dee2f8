"""Compiles the preparation kernels (sc-sfmlearner-release_amd/csrc_prep/*.hip), unchanged, against the host simulator
(tests/hostsim/hip/hip_runtime.h) with g++ into tests/hostsim/_build_prep/, and runs the C ABI of include/scsfm_prep.h on
HOST pointers.  Test infrastructure only; never loaded by the product."""
from __future__ import annotations

import ctypes
import functools
import os

import numpy as np

from hostsim import library
from scsfm_hip import prepare
from scsfm_hip._lib import PREP_ABI_VERSION, PREP_HEADER, CLib

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(ROOT, "sc-sfmlearner-release_amd", "csrc_prep")
HOSTSIM = os.path.join(HERE, "hostsim")
OUT = os.path.join(HOSTSIM, "_build_prep")
LIB = os.path.join(OUT, "libscsfm_prep_hostsim.so")


def build(force=False):
    return library.build("prep", force, dep=os.path.abspath(__file__))


@functools.lru_cache(maxsize=1)
def lib():
    return CLib(build(), PREP_HEADER, PREP_ABI_VERSION, "scsfm_prep_")


def _ptr(a):
    return ctypes.c_void_p(a.ctypes.data) if a is not None else None


def resize_u8(images, height, width, keep_rows=None):
    """scsfm_hip.prepare.resize_u8 on the simulator: uint8 [N, H, W, C] array -> uint8 [N, keep_rows, width, C].  The
    output starts as 0xAB so that a byte that is not stored shows."""
    L = lib()
    images = np.ascontiguousarray(images, np.uint8)
    N, H, W, C = images.shape
    plan = prepare.resize_plan(H, W, height, width, keep_rows)
    (hrows, htaps), (vrows, vtaps) = (t if t is not None else (None, None) for t in (plan["htab"], plan["vtab"]))
    both = hrows is not None and vrows is not None
    nbytes = L.size("scsfm_prep_resize_workspace_bytes", N, C, int(width), plan["src_rows"], int(both))
    ws = np.zeros(nbytes, np.uint8) if nbytes else None
    out = np.full((N, plan["keep"], int(width), C), 0xAB, np.uint8)
    L.call("scsfm_prep_resize_u8", N, H, W, C, plan["keep"], int(width), _ptr(images), _ptr(hrows), _ptr(htaps),
           0 if htaps is None else len(htaps), _ptr(vrows), _ptr(vtaps), 0 if vtaps is None else len(vtaps),
           plan["src_row0"], plan["src_rows"], _ptr(out), _ptr(ws), nbytes, None)
    return out


def velodyne_depth(points, scan_off, P, height, width, bounds):
    """scsfm_hip.prepare.velodyne_depth on the simulator, numpy arrays in and out.  The output starts as NaN."""
    L = lib()
    points = np.ascontiguousarray(points, np.float32).reshape(-1, 4)
    scan_off = np.ascontiguousarray(scan_off, np.int32)
    F = len(scan_off) - 1
    P = np.ascontiguousarray(P, np.float64).reshape(F, 3, 4)
    h, w = int(height), int(width)
    nbytes = L.size("scsfm_prep_velo_workspace_bytes", F, h, w)
    ws = np.full(max(nbytes, 1), 0x5A, np.uint8)  # (the library clears it itself)
    depth = np.full((F, h, w), np.nan, np.float32)
    L.call("scsfm_prep_velo_depth", F, h, w, float(bounds[0]), float(bounds[1]), _ptr(points) if len(points) else None,
           len(points), _ptr(scan_off), _ptr(P), _ptr(depth), _ptr(ws), nbytes, None)
    return depth
