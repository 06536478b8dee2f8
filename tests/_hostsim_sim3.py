"""Compiles the 7-DoF tracking kernels (sc-sfmlearner-release_amd/csrc_sim3/*.hip), unchanged, against the host simulator
(tests/hostsim/hip/hip_runtime.h) into tests/hostsim/_build_sim3/ and runs the C ABI of include/scsfm_sim3.h on HOST
pointers.  The row is not one of scsfm_hip.libraries.BY_NAME's, which tests/hostsim/library.py looks its rows up in, so
this module has the g++ line itself, as tests/_hostsim_track.py: library.py's flags, with -ffp-contract=off.  Outputs are
pre-filled with NaN and every array lies between two guard bands, which `_Call.run` checks after the call.  Test
infrastructure only; never loaded by the product."""
from __future__ import annotations

import functools
import glob
import os
import subprocess

import numpy as np

from scsfm_hip import build as build_py, libraries
from scsfm_hip._lib import SIM3_ABI_VERSION, SIM3_HEADER, CLib

from _hostsim_fuse import _Call as _FuseCall, _ptr

HERE = os.path.dirname(os.path.abspath(__file__))
HOSTSIM = os.path.join(HERE, "hostsim")
LIB = os.path.join(HOSTSIM, "_build_sim3", "libscsfm_sim3_hostsim.so")
FLAGS = ["-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-x", "c++", "-Wall", "-Wno-unused-function",
         "-Wno-unknown-pragmas"]


def sources():
    return sorted(glob.glob(os.path.join(libraries.find("sim3").csrc, "*.hip")))


def build(force=False):
    row = libraries.find("sim3")
    srcs = sources()
    deps = srcs + [os.path.join(HOSTSIM, "hip", "hip_runtime.h"), row.header, build_py.ICP_CORE, os.path.abspath(__file__)]
    if not force and os.path.exists(LIB) and all(os.path.getmtime(d) <= os.path.getmtime(LIB) for d in deps):
        return LIB
    os.makedirs(os.path.dirname(LIB), exist_ok=True)
    tmp = f"{LIB}.{os.getpid()}.tmp"
    subprocess.run(["g++", *FLAGS, "-shared", "-I", HOSTSIM, "-I", os.path.dirname(row.header), "-o", tmp, *srcs],
                   check=True)
    os.replace(tmp, LIB)
    return LIB


@functools.lru_cache(maxsize=1)
def lib():
    return CLib(build(), SIM3_HEADER, SIM3_ABI_VERSION, "scsfm_sim3_")


class _Call(_FuseCall):
    """tests/_hostsim_fuse.py's guarded arrays, run against this library"""

    def run(self, name, *args, status=0):
        rc = lib()._fn[name](*args)
        assert rc == status, f"{name} returned {rc}"
        self.check(name)


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b, a.dtype)
    return a.shape == b.shape and np.array_equal(a.view(np.uint8).reshape(-1), b.view(np.uint8).reshape(-1))


def init(c2w, scale0, K):
    """-> (state [V, 8] float64, est [V, 16] float32, sigma_f [V] float32)"""
    k = _Call()
    c2w = k.arg(np.ascontiguousarray(np.asarray(c2w, np.float64).reshape(-1, 12)))
    s0 = k.arg(np.ascontiguousarray(np.asarray(scale0, np.float64).reshape(len(c2w))))
    Kf = k.arg(np.ascontiguousarray(np.asarray(K, np.float32).reshape(9)))
    state, est, sigma_f = k.out((len(c2w), 8), np.float64), k.out((len(c2w), 16)), k.out((len(c2w),))
    k.run("scsfm_sim3_init", len(c2w), _ptr(c2w), _ptr(s0), _ptr(Kf), _ptr(state), _ptr(est), _ptr(sigma_f), None)
    return state.copy(), est.copy(), sigma_f.copy()


def poses(state):
    """-> (c2w [V, 3, 4], scale [V])"""
    k = _Call()
    state = k.arg(np.ascontiguousarray(state, np.float64))
    c2w, scale = k.out((len(state), 12), np.float64), k.out((len(state),), np.float64)
    k.run("scsfm_sim3_poses", len(state), _ptr(state), _ptr(c2w), _ptr(scale), None)
    return c2w.reshape(-1, 3, 4).copy(), scale.copy()


def scaled_depth(depth, sigma_f, is_disp, offset=0):
    """scsfm_sim3_scale; with ``offset`` both arrays start that many floats behind a 16-byte boundary (the scalar path)"""
    depth = np.ascontiguousarray(depth, np.float32)
    V, H, W = depth.shape
    k = _Call()
    d = k.arg(np.concatenate([np.zeros(offset, np.float32), depth.reshape(-1)]))[offset:]
    out = k.out((depth.size + offset,))[offset:]
    s = k.arg(np.ascontiguousarray(sigma_f, np.float32))
    assert d.ctypes.data % 16 == 4 * offset % 16 and out.ctypes.data % 16 == 4 * offset % 16
    k.run("scsfm_sim3_scale", V, H, W, _ptr(d), int(bool(is_disp)), _ptr(s), _ptr(out), None)
    assert _same(d, depth.reshape(-1)) and _same(s, sigma_f)
    return out.reshape(V, H, W).copy()


def align(depth, guess, scale0, K, ref_view, model_depth, model_normal, is_disp=True, near=0.0, max_depth=10.0,
          iterations=10, max_dist=0.3, min_pairs=64, min_scale_pivot=2e-3):
    """tests/sim3_oracle.py's align through the library: dict(state, est, sigma_f, c2w, scale, report, slab)"""
    depth = np.ascontiguousarray(depth, np.float32)
    V, H, W = depth.shape
    state, est, sigma_f = init(guess, scale0, K)
    k = _Call()
    d, ref = k.arg(depth), k.arg(np.ascontiguousarray(ref_view, np.float32).reshape(V, 16))
    M, N = k.arg(np.ascontiguousarray(model_depth, np.float32)), k.arg(np.ascontiguousarray(model_normal, np.float32))
    assert M.shape == (V, H, W) and N.shape == (V, 3, H, W)
    state, est, sigma_f = k.arg(state), k.arg(est), k.arg(sigma_f)
    n = lib().size("scsfm_sim3_ws_bytes", V, H, W)
    assert n == V * -(-H * W // 1024) * 37 * 8
    ws, report = k.out((n // 8,), np.float64), k.out((V, iterations, 6), np.float64)
    k.run("scsfm_sim3_iterate", V, H, W, _ptr(d), int(bool(is_disp)), float(np.float32(near)),
          float(np.float32(max_depth)), _ptr(ref), _ptr(M), _ptr(N), float(np.float32(max_dist)), int(min_pairs),
          float(min_scale_pivot), int(iterations), _ptr(state), _ptr(est), _ptr(sigma_f), _ptr(ws), _ptr(report), None)
    for got, want in ((d, depth), (ref, ref_view), (M, model_depth), (N, model_normal)):   # (the inputs are only read)
        assert _same(got.reshape(-1), np.ascontiguousarray(want, np.float32).reshape(-1))
    c2w, scale = poses(state)
    return dict(state=state.copy(), est=est.copy(), sigma_f=sigma_f.copy(), c2w=c2w, scale=scale, report=report.copy(),
                slab=ws.reshape(V, -1, 37).copy())
