"""Compiles the mesh kernels (sc-sfmlearner-release_amd/csrc_mesh/*.hip), unchanged, against the host simulator
(tests/hostsim/hip/hip_runtime.h, plus tests/hostsim/fuse_shim.h for the wave's ballot) into tests/hostsim/_build_mesh/ and
runs the C ABI of include/scsfm_mesh.h on HOST pointers.  The row is not one of scsfm_hip.libraries.BY_NAME's, which
tests/hostsim/library.py looks its rows up in, so this module has the g++ line itself, as tests/_hostsim_fuse.py:
library.py's flags, with -ffp-contract=off.  Outputs and the workspace are pre-filled with NaN (bytes and integers with
0xAB) and every array lies between two guard bands, which `_Call.run` checks after the call.  Test infrastructure only;
never loaded by the product."""
from __future__ import annotations

import ctypes
import functools
import glob
import os
import subprocess

import numpy as np

from scsfm_hip import libraries
from scsfm_hip._lib import MESH_ABI_VERSION, MESH_HEADER, CLib

from _hostsim_fuse import BYTE_FILL, _Call as _FuseCall, _ptr  # noqa: F401  (BYTE_FILL: for the tests)

HERE = os.path.dirname(os.path.abspath(__file__))
HOSTSIM = os.path.join(HERE, "hostsim")
SHIM = os.path.join(HOSTSIM, "fuse_shim.h")
LIB = os.path.join(HOSTSIM, "_build_mesh", "libscsfm_mesh_hostsim.so")


def build(force=False):
    row = libraries.find("mesh")
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
    return CLib(build(), MESH_HEADER, MESH_ABI_VERSION, "scsfm_mesh_")


class _Call(_FuseCall):
    """tests/_hostsim_fuse.py's guarded arrays, run against this library"""

    def run(self, name, *args, status=0):
        rc = lib()._fn[name](*args)
        assert rc == status, f"{name} returned {rc}"
        self.check(name)


def extract_mesh(planes, origin, voxel, min_weight=1.0, vertex_capacity=None, triangle_capacity=None):
    """scsfm_hip.meshing.extract_mesh on a numpy array of planes [5, nz, ny, nx] -> (xyz, rgb, tri, (V, T)).  With a
    capacity the arrays have that many rows; rows at and past the count keep their fill (NaN, 0xAB)."""
    planes = np.ascontiguousarray(planes, np.float32)
    _, nz, ny, nx = planes.shape
    k = _Call()
    vol = k.arg(planes)
    n = lib().size("scsfm_mesh_ws_bytes", nx, ny, nz)
    chunks = (nx * ny * nz + 1023) // 1024
    assert n >= 16 + 24 * chunks + 5 * nx * ny * nz and n % 16 == 0
    ws = k.out((n // 4,), np.int32)
    assert ws.ctypes.data % 16 == 0
    k.run("scsfm_mesh_count", nx, ny, nz, _ptr(vol), min_weight, _ptr(ws), n, None)
    v, t = (int(x) for x in ws[:4].view(np.int64))
    vcap = v if vertex_capacity is None else int(vertex_capacity)
    tcap = t if triangle_capacity is None else int(triangle_capacity)
    xyz, rgb, tri = k.out((vcap, 3)), k.out((vcap, 3), np.uint8), k.out((tcap, 3), np.int32)
    origin = [float(np.float32(o)) for o in origin]
    k.run("scsfm_mesh_vertices", nx, ny, nz, *origin, float(np.float32(voxel)), _ptr(vol), min_weight, _ptr(ws), n, v,
          vcap, _ptr(xyz) if vcap else None, _ptr(rgb) if vcap else None, None)
    k.run("scsfm_mesh_triangles", nx, ny, nz, _ptr(vol), min_weight, _ptr(ws), n, v, t, tcap,
          _ptr(tri) if tcap else None, None)
    assert np.array_equal(vol.view(np.uint32), planes.view(np.uint32))  # (the volume is only read)
    return xyz.copy(), rgb.copy(), tri.copy(), (v, t)
