"""Compiles the validation-log kernels (sc-sfmlearner-release_amd/csrc_vlog/*.hip), unchanged, against the host
simulator (tests/hostsim/hip/hip_runtime.h) with g++ into tests/hostsim/_build_vlog/, and runs the C ABI of
include/scsfm_vlog.h on HOST pointers.  Test infrastructure only; never loaded by the product."""
from __future__ import annotations

import ctypes
import functools
import os

import numpy as np

from hostsim import library
from scsfm_hip._lib import VLOG_ABI_VERSION, VLOG_HEADER, CLib

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(ROOT, "sc-sfmlearner-release_amd", "csrc_vlog")
HOSTSIM = os.path.join(HERE, "hostsim")
OUT = os.path.join(HOSTSIM, "_build_vlog")
LIB = os.path.join(OUT, "libscsfm_vlog_hostsim.so")


def build(force=False):
    return library.build("vlog", force, dep=os.path.abspath(__file__))


@functools.lru_cache(maxsize=1)
def lib():
    return CLib(build(), VLOG_HEADER, VLOG_ABI_VERSION, "scsfm_vlog_")


def _ptr(a):
    return ctypes.c_void_p(a.ctypes.data) if a is not None else None


def _aligned(shape, dtype, fill, offset=0):
    """An array whose first byte sits ``offset`` bytes past a 64-byte boundary, every byte ``fill``."""
    n = int(np.prod(shape)) * np.dtype(dtype).itemsize
    raw = np.full(n + 128, fill, np.uint8)
    start = (-raw.ctypes.data) % 64 + offset
    return raw[start:start + n].view(dtype).reshape(shape)


def _staged(a, offset):
    src = _aligned(a.shape, np.float32, 0, offset)
    src[...] = a
    return src


def input_pictures(batch, floats=True, bytes_=True, offset=0):
    """scsfm_hip.validation_log.input_pictures on the simulator, numpy in and out.  The outputs start as 0xAB bytes;
    ``offset`` (a multiple of 4) moves every buffer off the 16-byte boundary."""
    N, _, H, W = batch.shape
    src = _staged(batch, offset)
    out_f = _aligned((N, 3, H, W), np.float32, 0xAB, offset) if floats else None
    out_b = _aligned((N, H, W, 3), np.uint8, 0xAB, offset) if bytes_ else None
    lib().call("scsfm_vlog_input_picture", N, H, W, _ptr(src), _ptr(out_f), _ptr(out_b), None)
    return out_f, out_b


def target_disparity(depth, offset=0):
    N, H, W = depth.shape
    src = _staged(depth, offset)
    out = _aligned((N, H, W), np.float32, 0xAB, offset)
    lib().call("scsfm_vlog_target_disparity", N, H * W, _ptr(src), _ptr(out), None)
    assert np.array_equal(src, depth, equal_nan=True)  # (the input is not written)
    return out


def image_max(maps, offset=0):
    N, H, W = maps.shape
    src = _staged(maps, offset)
    out = _aligned((N,), np.float32, 0xAB, offset)
    lib().call("scsfm_vlog_image_max", N, H * W, _ptr(src), _ptr(out), None)
    return out


def map_pictures(maps, table, max_value=None, floats=True, bytes_=True, offset=0):
    """scsfm_hip.validation_log.map_pictures on the simulator with the float32 [table_n, 4] ``table``."""
    N, H, W = maps.shape
    src = _staged(maps, offset)
    tab = _staged(np.asarray(table, np.float32), 0)  # (one 16-byte word per entry: always aligned)
    divisors = image_max(src, offset) if max_value is None else None
    out_f = _aligned((N, 4, H, W), np.float32, 0xAB, offset) if floats else None
    out_b = _aligned((N, H, W, 4), np.uint8, 0xAB, offset) if bytes_ else None
    lib().call("scsfm_vlog_map_picture", N, H, W, _ptr(src), _ptr(tab), len(tab), _ptr(divisors),
               0.0 if max_value is None else float(max_value), _ptr(out_f), _ptr(out_b), None)
    return out_f, out_b
