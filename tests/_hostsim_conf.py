"""Compiles the confidence kernels (sc-sfmlearner-release_amd/csrc_conf/*.hip), unchanged, against the host simulator
(tests/hostsim/hip/hip_runtime.h, plus tests/hostsim/fuse_shim.h for the wave's ballot of the integration's cull) into
tests/hostsim/_build_conf/ and runs the C ABI of include/scsfm_conf.h on HOST pointers.  The row is not one of
scsfm_hip.libraries.BY_NAME's, which tests/hostsim/library.py looks its rows up in, so this module has the g++ line itself,
as tests/_hostsim_track.py: library.py's flags, with -ffp-contract=off.  Outputs are pre-filled with NaN and every array
lies between two guard bands, which `_Call.run` checks after the call; the inputs' bits are compared after it.  `Volume`
is tests/_hostsim_fuse.py's with the ``weight=`` keyword of scsfm_hip.fusion.Volume.integrate.  Test infrastructure only;
never loaded by the product."""
from __future__ import annotations

import functools
import glob
import os
import subprocess

import numpy as np

import _hostsim_fuse as HF
from _hostsim_fuse import _Call as _FuseCall, _ptr
from scsfm_hip import libraries
from scsfm_hip._lib import CONF_ABI_VERSION, CONF_HEADER, CLib

HERE = os.path.dirname(os.path.abspath(__file__))
HOSTSIM = os.path.join(HERE, "hostsim")
SHIM = os.path.join(HOSTSIM, "fuse_shim.h")
LIB = os.path.join(HOSTSIM, "_build_conf", "libscsfm_conf_hostsim.so")
FLAGS = ["-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-x", "c++", "-Wall", "-Wno-unused-function",
         "-Wno-unknown-pragmas"]
REDUCE = {"mean": 0, "max": 1}


def sources():
    return sorted(glob.glob(os.path.join(libraries.find("conf").csrc, "*.hip")))


def build(force=False):
    row = libraries.find("conf")
    srcs = sources()
    deps = srcs + [os.path.join(HOSTSIM, "hip", "hip_runtime.h"), SHIM, row.header, os.path.abspath(__file__)]
    if not force and os.path.exists(LIB) and all(os.path.getmtime(d) <= os.path.getmtime(LIB) for d in deps):
        return LIB
    os.makedirs(os.path.dirname(LIB), exist_ok=True)
    tmp = f"{LIB}.{os.getpid()}.tmp"
    subprocess.run(["g++", *FLAGS, "-shared", "-I", HOSTSIM, "-I", os.path.dirname(row.header), "-include", SHIM, "-o", tmp,
                    *srcs], check=True)
    os.replace(tmp, LIB)
    return LIB


@functools.lru_cache(maxsize=1)
def lib():
    return CLib(build(), CONF_HEADER, CONF_ABI_VERSION, "scsfm_conf_")


def _same(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


class _Call(_FuseCall):
    """tests/_hostsim_fuse.py's guarded arrays, run against this library"""

    def run(self, name, *args, status=0):
        rc = lib()._fn[name](*args)
        assert rc == status, f"{name} returned {rc}"
        self.check(name)


def pairs(c2w, K, radius):
    """-> pair [n, 2 radius, 16] float32"""
    k = _Call()
    src = np.ascontiguousarray(np.asarray(c2w, np.float64).reshape(-1, 12))
    c, Kf = k.arg(src), k.arg(np.ascontiguousarray(np.asarray(K, np.float32).reshape(9)))
    out = k.out((len(c), 2 * radius, 16))
    k.run("scsfm_conf_pairs", len(c), int(radius), _ptr(c), _ptr(Kf), _ptr(out), None)
    assert _same(c, src)
    return out.copy()


def weights(depth, pair, is_disp=True, max_depth=10.0, min_views=1, floor=0.0, reduce="mean"):
    """-> weight [n, H, W] float32"""
    depth = np.ascontiguousarray(depth, np.float32)
    pair = np.ascontiguousarray(pair, np.float32)
    n, H, W = depth.shape
    k = _Call()
    d, p = k.arg(depth), k.arg(pair)
    out = k.out((n, H, W))
    k.run("scsfm_conf_weights", n, pair.shape[1] // 2, H, W, _ptr(d), int(bool(is_disp)), _ptr(p),
          float(np.float32(max_depth)), int(min_views), float(np.float32(floor)), REDUCE[reduce], _ptr(out), None)
    assert _same(d, depth) and _same(p, pair)   # (the inputs are only read)
    return out.copy()


class Volume(HF.Volume):
    def integrate(self, depth, images, c2w, K, is_disp=True, near=0.0, max_depth=10.0, weight=None):
        if weight is None:
            return super().integrate(depth, images, c2w, K, is_disp, near, max_depth)
        depth = np.ascontiguousarray(depth, np.float32)
        weight = np.ascontiguousarray(weight, np.float32)
        F, H, W = depth.shape
        assert weight.shape == depth.shape
        cam = HF.cameras(c2w, K)
        assert len(cam) == F
        for f0 in range(0, F, self.frames_per_launch):
            f1 = min(F, f0 + self.frames_per_launch)
            k = _Call()
            d, w = k.arg(depth[f0:f1]), k.arg(weight[f0:f1])
            img = None if images is None else k.arg(np.ascontiguousarray(images[f0:f1], np.float32))
            c = k.arg(cam[f0:f1])
            k.run("scsfm_conf_integrate", *self.dims, *self.origin, self.voxel, self.trunc, near, max_depth,
                  self.max_weight, f1 - f0, H, W, _ptr(c), _ptr(d), _ptr(w), int(is_disp), _ptr(img), _ptr(self.planes),
                  None)
            self._k.check("scsfm_conf_integrate")  # (the volume's own bands)
            assert _same(d, depth[f0:f1]) and _same(w, weight[f0:f1]) and _same(c, cam[f0:f1])
            assert images is None or _same(img, np.ascontiguousarray(images[f0:f1], np.float32))
