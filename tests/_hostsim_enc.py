"""Compiles the encoder kernels (sc-sfmlearner-release_amd/csrc_enc/*.hip), unchanged, against the host simulator
(tests/hostsim/hip/hip_runtime.h) with g++ into tests/hostsim/_build_enc/, and runs the C ABI of include/scsfm_enc.h on
HOST pointers.  Every output is pre-filled with NaN.  Test infrastructure only; never loaded by the product."""
from __future__ import annotations

import ctypes
import functools
import os

import numpy as np

from hostsim import library
from scsfm_hip._lib import ENC_ABI_VERSION, ENC_HEADER, CLib

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(ROOT, "sc-sfmlearner-release_amd", "csrc_enc")
HOSTSIM = os.path.join(HERE, "hostsim")
OUT = os.path.join(HOSTSIM, "_build_enc")
LIB = os.path.join(OUT, "libscsfm_enc_hostsim.so")


def build(force=False):
    return library.build("enc", force, dep=os.path.abspath(__file__))


@functools.lru_cache(maxsize=1)
def lib():
    return CLib(build(), ENC_HEADER, ENC_ABI_VERSION, "scsfm_enc_")


def _ptr(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def _f32(a):
    return None if a is None else np.ascontiguousarray(a, np.float32)


def _nan(shape):
    return np.full(shape, np.nan, np.float32)


def _ws(L, shape):
    n = L.size("scsfm_enc_bn_workspace_bytes", *shape)
    return np.full(n // 8, np.nan), n


def bn_fwd(x, identity, gamma, beta, running_mean, running_var, nbt, mode, eps, momentum):
    """-> y, stat[3, C]; running_mean / running_var (float32 arrays) and nbt (int64[1]) are updated in place"""
    L = lib()
    x, identity, gamma, beta = _f32(x), _f32(identity), _f32(gamma), _f32(beta)
    B, C, H, W = x.shape
    y, stat = _nan(x.shape), _nan((3, C))
    ws, n = _ws(L, x.shape)
    L.call("scsfm_enc_bn_fwd_f32", B, C, H, W, mode, eps, momentum, _ptr(x), _ptr(identity), _ptr(gamma), _ptr(beta),
           _ptr(y), _ptr(stat), _ptr(running_mean), _ptr(running_var), _ptr(nbt), _ptr(ws), n, None)
    return y, stat


def bn_bwd(g, x, y, gamma, beta, stat, mode):
    """-> dx, d_identity (None unless mode 2), dgamma, dbeta"""
    L = lib()
    g, x, y, gamma, beta = _f32(g), _f32(x), _f32(y), _f32(gamma), _f32(beta)
    B, C, H, W = x.shape
    dx, d_id = _nan(x.shape), (_nan(x.shape) if mode == 2 else None)
    dgamma, dbeta = _nan(C), _nan(C)
    ws, n = _ws(L, x.shape)
    L.call("scsfm_enc_bn_bwd_f32", B, C, H, W, mode, _ptr(g), _ptr(x), _ptr(y if mode == 2 else None), _ptr(gamma),
           _ptr(beta), _ptr(stat), _ptr(dx), _ptr(d_id), _ptr(dgamma), _ptr(dbeta), _ptr(ws), n, None)
    return dx, d_id, dgamma, dbeta


def maxpool_fwd(x):
    x = _f32(x)
    B, C, H, W = x.shape
    shape = (B, C, (H - 1) // 2 + 1, (W - 1) // 2 + 1)
    out, arg = _nan(shape), np.full(shape, 255, np.uint8)
    lib().call("scsfm_enc_maxpool_fwd_f32", B, C, H, W, _ptr(x), _ptr(out), _ptr(arg), None)
    return out, arg


def maxpool_bwd(g, arg, shape):
    g = _f32(g)
    dx = _nan(shape)
    lib().call("scsfm_enc_maxpool_bwd_f32", *shape, _ptr(g), _ptr(arg), _ptr(dx), None)
    return dx
