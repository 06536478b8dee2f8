"""Compiles the eval-mode encoder kernels (sc-sfmlearner-release_amd/csrc_enceval/*.hip), unchanged, against the host
simulator (tests/hostsim/hip/hip_runtime.h) with g++ into tests/hostsim/_build_enceval/, and runs the C ABI of
include/scsfm_enceval.h on HOST pointers.  Every buffer handed to the library starts on a 64-byte boundary (so the shape
alone decides between the 16-byte and the scalar path); every output lies between two guard bands of a sentinel bit
pattern, is pre-filled with it, and the bands are checked after the call.  Test infrastructure only; never loaded by the
product."""
from __future__ import annotations

import ctypes
import functools
import os

import numpy as np

from hostsim import library
from scsfm_hip._lib import ENCEVAL_ABI_VERSION, ENCEVAL_HEADER, CLib

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(ROOT, "sc-sfmlearner-release_amd", "csrc_enceval")
HOSTSIM = os.path.join(HERE, "hostsim")
OUT = os.path.join(HOSTSIM, "_build_enceval")
LIB = os.path.join(OUT, "libscsfm_enceval_hostsim.so")
GUARD = 64              # floats on either side of an output
SENTINEL = 0x7FC0DEAD   # a NaN no kernel computes


def build(force=False):
    return library.build("enceval", force, dep=os.path.abspath(__file__))


@functools.lru_cache(maxsize=1)
def lib():
    return CLib(build(), ENCEVAL_HEADER, ENCEVAL_ABI_VERSION, "scsfm_enceval_")


def _aligned(shape, guard=0):
    """-> (raw, view): a float32 view of ``shape`` that starts on a 64-byte boundary, ``guard`` floats inside ``raw``"""
    n = int(np.prod(shape))
    raw = np.empty(n + 2 * guard + 16, np.float32)
    skip = (-(raw.ctypes.data + 4 * guard) % 64) // 4
    view = raw[skip + guard:skip + guard + n].reshape(shape)
    assert view.ctypes.data % 64 == 0
    return raw, view


def _in(a):
    if a is None:
        return None
    _, view = _aligned(np.shape(a))
    view[...] = a
    return view


class _Out:
    def __init__(self, shape):
        self.raw, self.view = _aligned(shape, GUARD)
        self.raw.view(np.int32)[...] = SENTINEL
        self.lo = (self.view.ctypes.data - self.raw.ctypes.data) // 4

    def finish(self, name):
        bits = self.raw.view(np.int32)
        assert np.all(bits[:self.lo] == SENTINEL) and np.all(bits[self.lo + self.view.size:] == SENTINEL), \
            f"{name}: a guard band was written"
        assert not np.any(self.view.view(np.int32) == SENTINEL), f"{name}: an entry was not stored"
        return self.view.copy()


def _ptr(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def bn(x, identity, gamma, beta, running_mean, running_var, mode, eps):
    """-> y; the per-channel vectors are handed over as they are (float32 arrays: the test checks they stay unchanged)"""
    x, identity = _in(x), _in(identity)
    B, C, H, W = x.shape
    y = _Out(x.shape)
    lib().call("scsfm_enceval_bn_f32", B, C, H, W, mode, eps, _ptr(x), _ptr(identity), _ptr(gamma), _ptr(beta),
               _ptr(running_mean), _ptr(running_var), _ptr(y.view), None)
    return y.finish("y")


def bn_relu_pool(x, gamma, beta, running_mean, running_var, eps):
    """-> f0, pooled"""
    x = _in(x)
    B, C, H, W = x.shape
    f0, pooled = _Out(x.shape), _Out((B, C, (H - 1) // 2 + 1, (W - 1) // 2 + 1))
    lib().call("scsfm_enceval_bn_relu_pool_f32", B, C, H, W, eps, _ptr(x), _ptr(gamma), _ptr(beta), _ptr(running_mean),
               _ptr(running_var), _ptr(f0.view), _ptr(pooled.view), None)
    return f0.finish("f0"), pooled.finish("pooled")


def maxpool(x):
    x = _in(x)
    B, C, H, W = x.shape
    out = _Out((B, C, (H - 1) // 2 + 1, (W - 1) // 2 + 1))
    lib().call("scsfm_enceval_maxpool_f32", B, C, H, W, _ptr(x), _ptr(out.view), None)
    return out.finish("out")
