"""Compiles the ray-cast kernels (sc-sfmlearner-release_amd/csrc_cast/*.hip), unchanged, against the host simulator
(tests/hostsim/hip/hip_runtime.h) into tests/hostsim/_build_cast/ and runs the C ABI of include/scsfm_cast.h on HOST
pointers.  The row is not one of scsfm_hip.libraries.BY_NAME's, which tests/hostsim/library.py looks its rows up in, so
this module has the g++ line itself, as tests/_hostsim_mesh.py: library.py's flags, with -ffp-contract=off.  Outputs are
pre-filled with NaN (bytes with 0xAB) and every array lies between two guard bands, which `_Call.run` checks after the
call.  Test infrastructure only; never loaded by the product."""
from __future__ import annotations

import functools
import glob
import os
import subprocess

import numpy as np

from scsfm_hip import libraries
from scsfm_hip._lib import CAST_ABI_VERSION, CAST_HEADER, CLib

from _hostsim_fuse import BYTE_FILL, _Call as _FuseCall, _ptr  # noqa: F401  (BYTE_FILL: for the tests)

HERE = os.path.dirname(os.path.abspath(__file__))
HOSTSIM = os.path.join(HERE, "hostsim")
LIB = os.path.join(HOSTSIM, "_build_cast", "libscsfm_cast_hostsim.so")
FLAGS = ["-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-x", "c++", "-Wall", "-Wno-unused-function",
         "-Wno-unknown-pragmas"]


def sources():
    return sorted(glob.glob(os.path.join(libraries.find("cast").csrc, "*.hip")))


def build(force=False):
    row = libraries.find("cast")
    srcs = sources()
    deps = srcs + [os.path.join(HOSTSIM, "hip", "hip_runtime.h"), row.header, os.path.abspath(__file__)]
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
    return CLib(build(), CAST_HEADER, CAST_ABI_VERSION, "scsfm_cast_")


class _Call(_FuseCall):
    """tests/_hostsim_fuse.py's guarded arrays, run against this library"""

    def run(self, name, *args, status=0):
        rc = lib()._fn[name](*args)
        assert rc == status, f"{name} returned {rc}"
        self.check(name)


def views(c2w, K):
    k = _Call()
    c2w = k.arg(np.ascontiguousarray(np.asarray(c2w, np.float64).reshape(-1, 12)))
    Kf = k.arg(np.ascontiguousarray(np.asarray(K, np.float32).reshape(9)))
    view = k.out((len(c2w), 16))
    k.run("scsfm_cast_views", len(c2w), _ptr(c2w), _ptr(Kf), _ptr(view), None)
    return view.copy()


def brick_mask(planes, min_weight=1.0):
    planes = np.ascontiguousarray(planes, np.float32)
    _, nz, ny, nx = planes.shape
    k = _Call()
    vol = k.arg(planes)
    n = lib().size("scsfm_cast_mask_bytes", nx, ny, nz)
    assert n == -(-nx // 8) * -(-ny // 8) * -(-nz // 8)
    mask = k.out((n,), np.uint8)
    k.run("scsfm_cast_mask", nx, ny, nz, _ptr(vol), min_weight, _ptr(mask), None)
    return mask.copy()


def cast(planes, origin, voxel, view, hw, near, step, n_steps, min_weight=1.0, mask=None, normals=True, colour=True,
         shade=True):
    """-> dict(depth, normal, rgb, shade) of numpy arrays (None for an output that was not asked for); `view` is the
    records [V, 16] as given (so that a test can put a NaN into one), `mask` the bytes or None"""
    planes = np.ascontiguousarray(planes, np.float32)
    _, nz, ny, nx = planes.shape
    H, W = hw
    V = len(view)
    k = _Call()
    vol = k.arg(planes)
    rec = k.arg(np.ascontiguousarray(view, np.float32))
    mk = None if mask is None else k.arg(np.ascontiguousarray(mask, np.uint8))
    depth = k.out((V, H, W))
    normal = k.out((V, 3, H, W)) if normals else None
    rgb = k.out((V, H, W, 3), np.uint8) if colour else None
    sh = k.out((V, H, W), np.uint8) if shade else None
    origin = [float(np.float32(o)) for o in origin]
    k.run("scsfm_cast_cast", nx, ny, nz, *origin, float(np.float32(voxel)), _ptr(vol), float(min_weight),
          float(np.float32(near)), float(np.float32(step)), int(n_steps), V, H, W, _ptr(rec), _ptr(mk), _ptr(depth),
          _ptr(normal), _ptr(rgb), _ptr(sh), None)
    assert np.array_equal(vol.view(np.uint32), planes.view(np.uint32))  # (the volume is only read)
    return {key: None if a is None else a.copy() for key, a in
            (("depth", depth), ("normal", normal), ("rgb", rgb), ("shade", sh))}
