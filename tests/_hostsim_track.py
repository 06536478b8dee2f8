"""Compiles the tracking kernels (sc-sfmlearner-release_amd/csrc_track/*.hip), unchanged, against the host simulator
(tests/hostsim/hip/hip_runtime.h) into tests/hostsim/_build_track/ and runs the C ABI of include/scsfm_track.h on HOST
pointers.  The row is not one of scsfm_hip.libraries.BY_NAME's, which tests/hostsim/library.py looks its rows up in, so
this module has the g++ line itself, as tests/_hostsim_cast.py: library.py's flags, with -ffp-contract=off.  Outputs are
pre-filled with NaN and every array lies between two guard bands, which `_Call.run` checks after the call.  Test
infrastructure only; never loaded by the product."""
from __future__ import annotations

import functools
import glob
import os
import subprocess

import numpy as np

from scsfm_hip import build as build_py, libraries
from scsfm_hip._lib import TRACK_ABI_VERSION, TRACK_HEADER, CLib

from _hostsim_fuse import _Call as _FuseCall, _ptr

HERE = os.path.dirname(os.path.abspath(__file__))
HOSTSIM = os.path.join(HERE, "hostsim")
LIB = os.path.join(HOSTSIM, "_build_track", "libscsfm_track_hostsim.so")
FLAGS = ["-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-x", "c++", "-Wall", "-Wno-unused-function",
         "-Wno-unknown-pragmas"]


def sources():
    return sorted(glob.glob(os.path.join(libraries.find("track").csrc, "*.hip")))


def build(force=False):
    row = libraries.find("track")
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
    return CLib(build(), TRACK_HEADER, TRACK_ABI_VERSION, "scsfm_track_")


class _Call(_FuseCall):
    """tests/_hostsim_fuse.py's guarded arrays, run against this library"""

    def run(self, name, *args, status=0):
        rc = lib()._fn[name](*args)
        assert rc == status, f"{name} returned {rc}"
        self.check(name)


def init(c2w, K):
    """-> (state [V, 7] float64, est [V, 16] float32)"""
    k = _Call()
    c2w = k.arg(np.ascontiguousarray(np.asarray(c2w, np.float64).reshape(-1, 12)))
    Kf = k.arg(np.ascontiguousarray(np.asarray(K, np.float32).reshape(9)))
    state, est = k.out((len(c2w), 7), np.float64), k.out((len(c2w), 16))
    k.run("scsfm_track_init", len(c2w), _ptr(c2w), _ptr(Kf), _ptr(state), _ptr(est), None)
    return state.copy(), est.copy()


def poses(state):
    k = _Call()
    state = k.arg(np.ascontiguousarray(state, np.float64))
    c2w = k.out((len(state), 12), np.float64)
    k.run("scsfm_track_poses", len(state), _ptr(state), _ptr(c2w), None)
    return c2w.reshape(-1, 3, 4).copy()


def align(depth, guess, K, ref_view, model_depth, model_normal, is_disp=True, near=0.0, max_depth=10.0, iterations=10,
          max_dist=0.3, min_pairs=64):
    """tests/track_oracle.py's align through the library: dict(state, est, c2w, report, slab)"""
    depth = np.ascontiguousarray(depth, np.float32)
    V, H, W = depth.shape
    state, est = init(guess, K)
    k = _Call()
    d, ref = k.arg(depth), k.arg(np.ascontiguousarray(ref_view, np.float32).reshape(V, 16))
    M, N = k.arg(np.ascontiguousarray(model_depth, np.float32)), k.arg(np.ascontiguousarray(model_normal, np.float32))
    assert M.shape == (V, H, W) and N.shape == (V, 3, H, W)
    state, est = k.arg(state), k.arg(est)
    n = lib().size("scsfm_track_ws_bytes", V, H, W)
    assert n == V * -(-H * W // 1024) * 29 * 8
    ws, report = k.out((n // 8,), np.float64), k.out((V, iterations, 4), np.float64)
    k.run("scsfm_track_iterate", V, H, W, _ptr(d), int(bool(is_disp)), float(np.float32(near)),
          float(np.float32(max_depth)), _ptr(ref), _ptr(M), _ptr(N), float(np.float32(max_dist)), int(min_pairs),
          int(iterations), _ptr(state), _ptr(est), _ptr(ws), _ptr(report), None)
    for got, want in ((d, depth), (ref, ref_view), (M, model_depth), (N, model_normal)):   # (the inputs are only read)
        assert np.array_equal(got.view(np.uint32).reshape(-1), np.ascontiguousarray(want, np.float32).view(np.uint32).reshape(-1))
    return dict(state=state.copy(), est=est.copy(), c2w=poses(state), report=report.copy(),
                slab=ws.reshape(V, -1, 29).copy())
