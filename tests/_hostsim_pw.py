"""Compiles the 1x1-convolution gradient kernels (sc-sfmlearner-release_amd/csrc_pw/*.hip), unchanged, against the host
simulator (tests/hostsim/hip/hip_runtime.h, plus tests/hostsim/wrw_shim.h for the fp32 matrix instruction, injected as
tests/_hostsim_wrw.py does) into tests/hostsim/_build_pw/ and runs the C ABI of include/scsfm_pw.h on HOST pointers.
The row is not one of scsfm_hip.libraries.BY_NAME's, which tests/hostsim/library.py looks its rows up in, so this module
has the g++ line itself, as tests/_hostsim_opt.py: library.py's flags.  Outputs and the workspace are pre-filled with NaN
(or with `fill`) and every array lies between two guard bands of NaN, which `_Call.run` checks after the call.  Test
infrastructure only; never loaded by the product."""
from __future__ import annotations

import functools
import glob
import os
import subprocess

import numpy as np

from _hostsim_wrw import _Call as _WrwCall, _ptr
from scsfm_hip import libraries
from scsfm_hip._lib import PW_ABI_VERSION, PW_HEADER, CLib

HERE = os.path.dirname(os.path.abspath(__file__))
HOSTSIM = os.path.join(HERE, "hostsim")
SHIM = os.path.join(HOSTSIM, "wrw_shim.h")
LIB = os.path.join(HOSTSIM, "_build_pw", "libscsfm_pw_hostsim.so")


def build(force=False):
    row = libraries.find("pw")
    srcs = sorted(glob.glob(os.path.join(row.csrc, "*.hip")))
    deps = srcs + [os.path.join(HOSTSIM, "hip", "hip_runtime.h"), SHIM, row.header, os.path.abspath(__file__)]
    if not force and os.path.exists(LIB) and all(os.path.getmtime(d) <= os.path.getmtime(LIB) for d in deps):
        return LIB
    os.makedirs(os.path.dirname(LIB), exist_ok=True)
    tmp = f"{LIB}.{os.getpid()}.tmp"
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-x", "c++", "-I", HOSTSIM,
                    "-I", os.path.dirname(row.header), "-include", SHIM, "-Wall", "-Wno-unused-function",
                    "-Wno-unknown-pragmas", "-o", tmp, *srcs], check=True)
    os.replace(tmp, LIB)
    return LIB


@functools.lru_cache(maxsize=1)
def lib():
    return CLib(build(), PW_HEADER, PW_ABI_VERSION, "scsfm_pw_")


class _Call(_WrwCall):
    def run(self, name, *args, status=0):
        rc = lib()._fn[name](*args)
        assert rc == status, f"{name} returned {rc}"
        assert all(np.isnan(b).all() for b in self.bands), f"{name} wrote outside its arrays"


def out_size(n, stride):
    return (n - 1) // stride + 1


def ws_bytes(B, Cin, Cout, H, W, stride):
    return lib().size("scsfm_pw_wrw_ws_bytes", B, Cin, Cout, H, W, stride)


def wrw(x, dy, stride, fill=np.nan):
    """-> dw[Cout, Cin], ws: x [B, Cin, H, W], dy [B, Cout, Ho, Wo]"""
    k = _Call()
    B, Cin, H, W = x.shape
    Cout = dy.shape[1]
    assert dy.shape == (B, Cout, out_size(H, stride), out_size(W, stride))
    x, dy = k.arg(x), k.arg(dy)
    n = ws_bytes(B, Cin, Cout, H, W, stride)
    assert n > 0 and n % (4 * Cout * Cin) == 0
    dw, ws = k.out((Cout, Cin), fill), k.out((n // 4,), fill)
    k.run("scsfm_pw_wrw_f32", B, Cin, Cout, H, W, stride, _ptr(x), _ptr(dy), _ptr(dw), _ptr(ws), n, None)
    return dw, ws


def dgrad(dy, w, H, W, fill=np.nan):
    """-> dx[B, Cin, H, W] of the stride-2 convolution: dy [B, Cout, Ho, Wo], w [Cout, Cin]"""
    k = _Call()
    B, Cout = dy.shape[:2]
    Cin = w.shape[1]
    assert dy.shape == (B, Cout, out_size(H, 2), out_size(W, 2)) and w.shape == (Cout, Cin)
    dy, w = k.arg(dy), k.arg(w)
    dx = k.out((B, Cin, H, W), fill)
    k.run("scsfm_pw_dgrad_f32", B, Cin, Cout, H, W, _ptr(dy), _ptr(w), _ptr(dx), None)
    return dx
