"""Compiles the fusion kernels (sc-sfmlearner-release_amd/csrc_fuse/*.hip), unchanged, against the host simulator
(tests/hostsim/hip/hip_runtime.h, plus tests/hostsim/fuse_shim.h for the wave's ballot) into tests/hostsim/_build_fuse/ and
runs the C ABI of include/scsfm_fuse.h on HOST pointers.  The row is not one of scsfm_hip.libraries.BY_NAME's, which
tests/hostsim/library.py looks its rows up in, so this module has the g++ line itself, as tests/_hostsim_pw.py:
library.py's flags.  Outputs and the workspace are pre-filled with NaN (bytes with 0xAB) and every array lies between two
guard bands, which `_Call.run` checks after the call.  `Volume` mirrors scsfm_hip.fusion.Volume's calls on numpy arrays,
so that tests/_fusion_cases.py drives both.  Test infrastructure only; never loaded by the product."""
from __future__ import annotations

import ctypes
import functools
import glob
import os
import subprocess

import numpy as np

from scsfm_hip import libraries
from scsfm_hip._lib import FUSE_ABI_VERSION, FUSE_HEADER, CLib

HERE = os.path.dirname(os.path.abspath(__file__))
HOSTSIM = os.path.join(HERE, "hostsim")
SHIM = os.path.join(HOSTSIM, "fuse_shim.h")
LIB = os.path.join(HOSTSIM, "_build_fuse", "libscsfm_fuse_hostsim.so")
GUARD = 4096
BYTE_FILL = 0xAB


def build(force=False):
    row = libraries.find("fuse")
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
    return CLib(build(), FUSE_HEADER, FUSE_ABI_VERSION, "scsfm_fuse_")


def _ptr(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


class _Call:
    """the arrays of one call, each inside a buffer of its own between two guard bands; run() checks every band"""

    def __init__(self):
        self.bands = []

    def _place(self, shape, dtype):
        n = int(np.prod(shape))
        dtype = np.dtype(dtype)
        fill = np.nan if dtype.kind == "f" else BYTE_FILL
        # (a multiple of 16 bytes in front, so that an array starts as aligned as numpy's allocation)
        buf = np.full(n + 2 * GUARD, fill, dtype)
        self.bands += [(buf[:GUARD], fill), (buf[GUARD + n:], fill)]
        return buf[GUARD:GUARD + n].reshape(shape)

    def arg(self, a):
        v = self._place(a.shape, a.dtype)
        v[...] = a
        return v

    def out(self, shape, dtype=np.float32):
        return self._place(shape, dtype)

    def run(self, name, *args, status=0):
        rc = lib()._fn[name](*args)
        assert rc == status, f"{name} returned {rc}"
        self.check(name)

    def check(self, name):
        for band, fill in self.bands:
            ok = np.isnan(band).all() if isinstance(fill, float) else (band == fill).all()
            assert ok, f"{name} wrote outside its arrays"


def cameras(c2w, K):
    """-> cam [n, 16] float32: c2w [n, 12] (or [n, 3, 4]) float64, K [3, 3] float32"""
    k = _Call()
    c2w = k.arg(np.ascontiguousarray(np.asarray(c2w, np.float64).reshape(-1, 12)))
    Kf = k.arg(np.ascontiguousarray(np.asarray(K, np.float32).reshape(9)))
    cam = k.out((len(c2w), 16))
    k.run("scsfm_fuse_cameras", len(c2w), _ptr(c2w), _ptr(Kf), _ptr(cam), None)
    return cam.copy()


class Volume:
    """scsfm_hip.fusion.Volume on numpy arrays over the simulator: the five planes live in one guarded buffer that every
    call reads and writes in place."""

    def __init__(self, dims, origin, voxel_size, trunc=None, max_weight=64.0, frames_per_launch=8):
        self.dims = tuple(int(d) for d in dims)
        self.origin = tuple(float(np.float32(o)) for o in origin)
        self.voxel = float(np.float32(voxel_size))
        self.trunc = float(np.float32(3 * voxel_size if trunc is None else trunc))
        self.max_weight = float(max_weight)
        self.frames_per_launch = int(frames_per_launch)
        nx, ny, nz = self.dims
        assert lib().size("scsfm_fuse_volume_bytes", nx, ny, nz) == 20 * nx * ny * nz
        self._k = _Call()
        self.planes = self._k.out((5, nz, ny, nx))
        self.planes[...] = 0

    tsdf = property(lambda self: self.planes[0])
    weight = property(lambda self: self.planes[1])
    colour = property(lambda self: self.planes[2:])

    def integrate(self, depth, images, c2w, K, is_disp=True, near=0.0, max_depth=10.0):
        depth = np.ascontiguousarray(depth, np.float32)
        F, H, W = depth.shape
        cam = cameras(c2w, K)
        assert len(cam) == F
        for f0 in range(0, F, self.frames_per_launch):
            f1 = min(F, f0 + self.frames_per_launch)
            k = _Call()
            d = k.arg(depth[f0:f1])
            img = None if images is None else k.arg(np.ascontiguousarray(images[f0:f1], np.float32))
            c = k.arg(cam[f0:f1])
            k.run("scsfm_fuse_integrate", *self.dims, *self.origin, self.voxel, self.trunc, near, max_depth,
                  self.max_weight, f1 - f0, H, W, _ptr(c), _ptr(d), int(is_disp), _ptr(img), _ptr(self.planes), None)
            self._k.check("scsfm_fuse_integrate")  # (the volume's own bands)

    def count(self, min_weight=1.0):
        """-> (the number of crossings, the workspace as ints)"""
        k = _Call()
        n = lib().size("scsfm_fuse_extract_ws_bytes", *self.dims)
        assert n > 0 and n % 4 == 0
        ws = k.out((n // 4,), np.int32)
        k.run("scsfm_fuse_count", *self.dims, _ptr(self.planes), min_weight, _ptr(ws), n, None)
        return int(ws[0]), ws

    def extract(self, min_weight=1.0, capacity=None):
        """-> (xyz [count, 3], rgb [count, 3]) or, with a capacity, the two buffers of that many rows (rows at and past
        the count keep their fill: NaN and 0xAB)"""
        total, ws = self.count(min_weight)
        cap = total if capacity is None else int(capacity)
        k = _Call()
        xyz, rgb = k.out((cap, 3)), k.out((cap, 3), np.uint8)
        k.run("scsfm_fuse_extract", *self.dims, *self.origin, self.voxel, _ptr(self.planes), min_weight, _ptr(ws),
              ws.nbytes, cap, _ptr(xyz) if cap else None, _ptr(rgb) if cap else None, None)
        return xyz.copy(), rgb.copy()
