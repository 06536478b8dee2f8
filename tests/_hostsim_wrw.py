"""Compiles the weight-gradient kernels (sc-sfmlearner-release_amd/csrc_wrw/*.hip), unchanged, against the host
simulator (tests/hostsim/hip/hip_runtime.h, plus tests/hostsim/wrw_shim.h for the fp32 matrix instruction) with g++ into
tests/hostsim/_build_wrw/, and runs the C ABI of include/scsfm_wrw.h on HOST pointers.  As in tests/_hostsim_nets.py the
output and the workspace are pre-filled with NaN (or with `fill`) and every array lies between two guard bands of NaN,
which `_Call.run` checks after the call.  `weight_grad` at the end stands in for scsfm_hip.conv_wrw's on CPU tensors.
Test infrastructure only; never loaded by the product."""
from __future__ import annotations

import ctypes
import functools
import os

import numpy as np
import torch

from hostsim import library
from scsfm_hip._lib import WRW_ABI_VERSION, WRW_HEADER, CLib

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(ROOT, "sc-sfmlearner-release_amd", "csrc_wrw")
HOSTSIM = os.path.join(HERE, "hostsim")
SHIM = os.path.join(HOSTSIM, "wrw_shim.h")
OUT = os.path.join(HOSTSIM, "_build_wrw")
LIB = os.path.join(OUT, "libscsfm_wrw_hostsim.so")
GUARD_MAX = 1 << 16


def build(force=False, src=SRC, lib=LIB):
    return library.build("wrw", force, src, lib, shim=SHIM, dep=os.path.abspath(__file__))


@functools.lru_cache(maxsize=1)
def lib():
    return CLib(build(), WRW_HEADER, WRW_ABI_VERSION, "scsfm_wrw_")


def ws_bytes(B, Cin, Cout, H, W):
    return lib().size("scsfm_wrw_conv3x3_ws_bytes", B, Cin, Cout, H, W)


def _ptr(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


class _Call:
    """the arrays of one call, each inside a NaN-filled buffer of its own; run() checks every band afterwards"""

    def __init__(self):
        self.bands = []

    def _place(self, shape, dtype=np.float32):
        n = int(np.prod(shape))
        g = min(n, GUARD_MAX) + 64
        buf = np.full(n + 2 * g, np.nan, dtype)
        self.bands += [buf[:g], buf[g + n:]]
        return buf[g:g + n].reshape(shape)

    def arg(self, a):
        v = self._place(a.shape)
        v[...] = a
        return v

    def out(self, shape, fill):
        v = self._place(shape)
        v[...] = fill
        return v

    def run(self, name, *args, status=0):
        rc = lib()._fn[name](*args)
        assert rc == status, f"{name} returned {rc}"
        assert all(np.isnan(b).all() for b in self.bands), f"{name} wrote outside its arrays"


def conv3x3_wrw(x, dy, fill=np.nan):
    """-> dw[Cout, Cin, 3, 3], ws: x is the padded [B, Cin, H + 2, W + 2], dy [B, Cout, H, W]"""
    k = _Call()
    B, Cin, Hp, Wp = x.shape
    _, Cout, H, W = dy.shape
    assert dy.shape[0] == B and (Hp, Wp) == (H + 2, W + 2)
    x, dy = k.arg(x), k.arg(dy)
    n = ws_bytes(B, Cin, Cout, H, W)
    assert n > 0 and n % 4 == 0
    dw, ws = k.out((Cout, Cin, 3, 3), fill), k.out((n // 4,), fill)
    k.run("scsfm_wrw_conv3x3_f32", B, Cin, Cout, H, W, _ptr(x), _ptr(dy), _ptr(dw), _ptr(ws), n, None)
    return dw, ws


CALLS = [0]


def weight_grad(x, gy):
    """scsfm_hip.conv_wrw.weight_grad on CPU fp32 tensors, over the simulator; CALLS counts the calls"""
    assert x.dtype == torch.float32 and not x.is_cuda and x.dim() == 4
    CALLS[0] += 1
    dw, _ = conv3x3_wrw(x.detach().contiguous().numpy(), gy.detach().contiguous().numpy())
    return torch.from_numpy(dw.copy())
