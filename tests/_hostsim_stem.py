"""Compiles the stem kernels (sc-sfmlearner-release_amd/csrc_stem/*.hip), unchanged, against the host simulator
(tests/hostsim/hip/hip_runtime.h) with g++ into tests/hostsim/_build_stem/, and runs the C ABI of include/scsfm_stem.h
on HOST pointers.  Every output is pre-filled with NaN (255 for the argmax).  Test infrastructure only; never loaded by
the product."""
from __future__ import annotations

import ctypes
import functools
import os

import numpy as np

from hostsim import library
from scsfm_hip._lib import STEM_ABI_VERSION, STEM_HEADER, CLib

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(ROOT, "sc-sfmlearner-release_amd", "csrc_stem")
HOSTSIM = os.path.join(HERE, "hostsim")
OUT = os.path.join(HOSTSIM, "_build_stem")
LIB = os.path.join(OUT, "libscsfm_stem_hostsim.so")


def build(force=False):
    return library.build("stem", force, dep=os.path.abspath(__file__))


@functools.lru_cache(maxsize=1)
def lib():
    return CLib(build(), STEM_HEADER, STEM_ABI_VERSION, "scsfm_stem_")


def _ptr(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def _f32(a):
    return None if a is None else np.ascontiguousarray(a, np.float32)


def _nan(shape):
    return np.full(shape, np.nan, np.float32)


def _ws(L, shape):
    n = L.size("scsfm_stem_workspace_bytes", *shape)
    return np.full(n // 8, np.nan), n


def pooled_shape(shape):
    B, C, H, W = shape
    return B, C, (H - 1) // 2 + 1, (W - 1) // 2 + 1


def fwd(x, gamma, beta, running_mean, running_var, nbt, eps, momentum):
    """-> f0, out, arg, stat[3, C]; running_mean / running_var (float32 arrays) and nbt (int64[1]) are updated in place"""
    L = lib()
    x, gamma, beta = _f32(x), _f32(gamma), _f32(beta)
    B, C, H, W = x.shape
    f0, stat = _nan(x.shape), _nan((3, C))
    out, arg = _nan(pooled_shape(x.shape)), np.full(pooled_shape(x.shape), 255, np.uint8)
    ws, n = _ws(L, x.shape)
    L.call("scsfm_stem_fwd_f32", B, C, H, W, eps, momentum, _ptr(x), _ptr(gamma), _ptr(beta), _ptr(f0), _ptr(out),
           _ptr(arg), _ptr(stat), _ptr(running_mean), _ptr(running_var), _ptr(nbt), _ptr(ws), n, None)
    return f0, out, arg, stat


def bwd(g_pool, g_f0, arg, x, gamma, beta, stat):
    """-> dx, dgamma, dbeta (g_f0 may be None)"""
    L = lib()
    g_pool, g_f0, x, gamma, beta = _f32(g_pool), _f32(g_f0), _f32(x), _f32(gamma), _f32(beta)
    arg, stat = np.ascontiguousarray(arg, np.uint8), _f32(stat)
    B, C, H, W = x.shape
    dx, dgamma, dbeta = _nan(x.shape), _nan(C), _nan(C)
    ws, n = _ws(L, x.shape)
    L.call("scsfm_stem_bwd_f32", B, C, H, W, _ptr(g_pool), _ptr(g_f0), _ptr(arg), _ptr(x), _ptr(gamma), _ptr(beta),
           _ptr(stat), _ptr(dx), _ptr(dgamma), _ptr(dbeta), _ptr(ws), n, None)
    return dx, dgamma, dbeta
