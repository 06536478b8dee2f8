"""Compiles the rolling-volume kernels (sc-sfmlearner-release_amd/csrc_roll/*.hip), unchanged, against the host simulator
(tests/hostsim/hip/hip_runtime.h, plus tests/hostsim/fuse_shim.h for the wave's ballot of the extraction) into
tests/hostsim/_build_roll/ and runs the C ABI of include/scsfm_roll.h on HOST pointers.  The row is not one of
scsfm_hip.libraries.BY_NAME's, which tests/hostsim/library.py looks its rows up in, so this module has the g++ line itself,
as tests/_hostsim_conf.py: library.py's flags, with -ffp-contract=off.  Outputs are pre-filled with NaN (bytes and ints with
0xAB) and every array lies between two guard bands, which `_Call.run` checks after the call; the inputs' bits are compared
after it.  `RollingVolume` is scsfm_hip.rolling.RollingVolume on numpy arrays over tests/_hostsim_fuse.py's Volume.  Test
infrastructure only; never loaded by the product."""
from __future__ import annotations

import functools
import glob
import os
import subprocess

import numpy as np

import _hostsim_fuse as HF
import rolling_oracle as RO
from _hostsim_fuse import _Call as _FuseCall, _ptr
from scsfm_hip import libraries
from scsfm_hip._lib import ROLL_ABI_VERSION, ROLL_HEADER, CLib

HERE = os.path.dirname(os.path.abspath(__file__))
HOSTSIM = os.path.join(HERE, "hostsim")
SHIM = os.path.join(HOSTSIM, "fuse_shim.h")
LIB = os.path.join(HOSTSIM, "_build_roll", "libscsfm_roll_hostsim.so")
FLAGS = ["-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-x", "c++", "-Wall", "-Wno-unused-function",
         "-Wno-unknown-pragmas"]


def sources():
    return sorted(glob.glob(os.path.join(libraries.find("roll").csrc, "*.hip")))


def build(force=False):
    row = libraries.find("roll")
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
    return CLib(build(), ROLL_HEADER, ROLL_ABI_VERSION, "scsfm_roll_")


def _same(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


class _Call(_FuseCall):
    """tests/_hostsim_fuse.py's guarded arrays, run against this library"""

    def run(self, name, *args, status=0):
        rc = lib()._fn[name](*args)
        assert rc == status, f"{name} returned {rc}"
        self.check(name)


def shift(planes, s, lead=0, status=0):
    """-> dst [5, nz, ny, nx]: the planes moved by s.  ``lead``: dst starts that many floats past numpy's alignment (the
    first and last group of four are then partial).  With a status of -1 the call must leave dst as it was (NaN)."""
    planes = np.ascontiguousarray(planes, np.float32)
    _, nz, ny, nx = planes.shape
    k = _Call()
    src = k.arg(planes)
    full = k.out((planes.size + lead,))
    dst = full[lead:]
    k.run("scsfm_roll_shift", nx, ny, nz, *(int(v) for v in s), _ptr(src), _ptr(dst), None, status=status)
    assert _same(src, planes), "the shift changed its source"
    assert np.isnan(full[:lead]).all(), "the shift wrote in front of dst"
    return dst.reshape(planes.shape).copy()


def leaving(planes, dims, origin, voxel, box, min_weight=1.0, capacity=None):
    """-> (the count, the workspace as ints, xyz [cap, 3], rgb [cap, 3]); rows at and past the count keep their fill"""
    planes = np.ascontiguousarray(planes, np.float32)
    k = _Call()
    vol = k.arg(planes)
    n = lib().size("scsfm_roll_ws_bytes", *dims)
    assert n > 0 and n % 4 == 0 and n == HF.lib().size("scsfm_fuse_extract_ws_bytes", *dims)
    ws = k.out((n // 4,), np.int32)
    k.run("scsfm_roll_count", *dims, *box, _ptr(vol), min_weight, _ptr(ws), n, None)
    total = int(ws[0])
    cap = total if capacity is None else int(capacity)
    xyz, rgb = k.out((cap, 3)), k.out((cap, 3), np.uint8)
    k.run("scsfm_roll_extract", *dims, *(float(np.float32(o)) for o in origin), float(np.float32(voxel)), *box, _ptr(vol),
          min_weight, _ptr(ws), n, cap, _ptr(xyz) if cap else None, _ptr(rgb) if cap else None, None)
    assert _same(vol, planes), "the extraction changed the volume"
    return total, ws.copy(), xyz.copy(), rgb.copy()


class RollingVolume(HF.Volume):
    """scsfm_hip.rolling.RollingVolume's calls on numpy arrays: two guarded buffers, ping-pong"""

    def __init__(self, dims, origin0, voxel_size, trunc=None, max_weight=64.0, frames_per_launch=8):
        super().__init__(dims, origin0, voxel_size, trunc, max_weight, frames_per_launch)
        self.origin0, self.offset = self.origin, (0, 0, 0)
        self._k2 = _Call()
        self._spare = self._k2.out(self.planes.shape)
        self._spare[...] = 0

    def shift(self, s, min_weight=1.0):
        s = tuple(int(v) for v in s)
        _, _, xyz, rgb = leaving(self.planes, self.dims, self.origin, self.voxel, RO.keep_box(self.dims, s), min_weight)
        nx, ny, nz = self.dims
        before = self.planes.copy()
        self._spare[...] = np.nan
        rc = lib()._fn["scsfm_roll_shift"](nx, ny, nz, *s, _ptr(self.planes), _ptr(self._spare), None)
        assert rc == 0
        self._k.check("scsfm_roll_shift")
        self._k2.check("scsfm_roll_shift")
        assert _same(before, self.planes)
        self.planes, self._spare = self._spare, self.planes
        self._k, self._k2 = self._k2, self._k
        self.offset = tuple(a + b for a, b in zip(self.offset, s))
        self.origin = tuple(float(o) for o in RO.origin_at(self.origin0, self.offset, self.voxel))
        return xyz, rgb
