"""The volumes and checks that tests/test_mesh_hostsim.py (host simulator) and tests/test_gpu_mesh.py (device) both use,
each against tests/mesh_oracle.py bit for bit.  A backend's `mesh(planes, origin, voxel, min_weight, vcap, tcap)` returns
numpy arrays (xyz, rgb, tri).  References are computed once (cached) and read-only.  Test infrastructure only."""
from __future__ import annotations

import functools

import numpy as np

import mesh_oracle as MO

f32 = np.float32
DIRECT_DIMS = (7, 5, 6)
DIRECT_ORIGIN = (0.1, -0.2, 0.3)
DIRECT_VOXEL = 0.1
DIRECT_MIN_WEIGHT = 2.0
DIRECT_SEED = 3


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _frozen(ref):
    for a in ref.values():
        a.setflags(write=False)
    return ref


@functools.lru_cache(maxsize=None)
def direct_planes(seed=DIRECT_SEED):
    """7 x 5 x 6 planes filled by hand: random tsdf in [-1, 1] with an exact 0.0 and a -0.0 (neither is "< 0"), a NaN,
    +1 and -1, and a negative voxel whose +x neighbour is 0.0 (frac == 1: a degenerate vertex at the edge's end); weights
    1 .. 3 scattered round the min_weight of 2; colours a little outside [0, 1]."""
    nx, ny, nz = DIRECT_DIMS
    rng = np.random.default_rng(seed)
    planes = np.zeros((5, nz, ny, nx), np.float32)
    planes[0] = rng.uniform(-1, 1, (nz, ny, nx)).astype(np.float32)
    planes[1] = rng.integers(1, 4, (nz, ny, nx)).astype(np.float32)
    planes[2:] = rng.uniform(-0.1, 1.1, (3, nz, ny, nx)).astype(np.float32)
    t, w = planes[0], planes[1]
    t[2, 2, 3], t[2, 2, 2] = 0.0, -0.4       # frac == -0.4 / (-0.4 - 0.0) == 1
    t[3, 1, 4], t[3, 1, 3] = -0.0, -0.25
    t[1, 3, 5], t[4, 2, 1], t[1, 1, 1] = np.nan, 1.0, -1.0
    w[2, 2, 2:4] = w[3, 1, 3:5] = 2
    w[1, 3, 5] = w[4, 2, 1] = w[1, 1, 1] = 3
    planes.setflags(write=False)
    return planes


@functools.lru_cache(maxsize=None)
def direct_reference(min_weight=DIRECT_MIN_WEIGHT):
    return _frozen(MO.mesh(direct_planes(), DIRECT_ORIGIN, DIRECT_VOXEL, min_weight))


# ---- the analytic sphere ----

SPHERE_N = 24
SPHERE_VOXEL = 0.1
SPHERE_R = 8 * SPHERE_VOXEL
SPHERE_TRUNC = 3 * SPHERE_VOXEL
# off the lattice, and chosen (on the oracle's mesh) so that no triangle's area is below 1e-6 voxel^2: the smallest is
# 5.4e-8 = 5.4e-6 voxel^2; the sphere lies trunc inside the box of the voxel centres
SPHERE_C = (1.2351, 1.1754, 1.2111)


@functools.lru_cache(maxsize=1)
def sphere_planes():
    """t = clip((|p - c| - R) / trunc, -1, 1) in fp32 at the voxel centres p, weight 1 everywhere, grey colour"""
    ax = MO.centres(0.0, SPHERE_N, SPHERE_VOXEL)
    assert min(SPHERE_C) - SPHERE_R - SPHERE_TRUNC >= ax[0] and max(SPHERE_C) + SPHERE_R + SPHERE_TRUNC <= ax[-1]
    z, y, x = np.meshgrid(ax, ax, ax, indexing="ij")
    cx, cy, cz = (f32(v) for v in SPHERE_C)
    d = np.sqrt((x - cx) * (x - cx) + (y - cy) * (y - cy) + (z - cz) * (z - cz))
    planes = np.zeros((5, SPHERE_N, SPHERE_N, SPHERE_N), np.float32)
    planes[0] = np.clip((d - f32(SPHERE_R)) / f32(SPHERE_TRUNC), f32(-1), f32(1))
    planes[1] = 1
    planes[2:] = 0.5
    assert planes.dtype == np.float32 and d.dtype == np.float32
    planes.setflags(write=False)
    return planes


@functools.lru_cache(maxsize=1)
def sphere_reference():
    return _frozen(MO.mesh(sphere_planes(), (0.0, 0.0, 0.0), SPHERE_VOXEL, 1.0))


def check_sphere(xyz, tri):
    """The mesh of the sphere is a closed oriented 2-manifold whose triangles face away from the centre and whose
    vertices lie on the sphere to the interpolation error."""
    xyz64, tri = xyz.astype(np.float64), tri.astype(np.int64)
    V, F = len(xyz), len(tri)
    assert F > 1000 and tri.min() >= 0 and tri.max() < V
    # every directed edge once, and its reverse once
    directed = np.concatenate([tri[:, [0, 1]], tri[:, [1, 2]], tri[:, [2, 0]]])
    key = directed[:, 0] * V + directed[:, 1]
    assert len(np.unique(key)) == len(key), "a directed edge occurs twice"
    assert np.array_equal(np.sort(key), np.sort(directed[:, 1] * V + directed[:, 0])), "an edge without its reverse"
    assert (directed[:, 0] != directed[:, 1]).all()
    used = np.unique(tri)
    assert len(used) == V, "a vertex that no triangle uses"
    E = len(key) // 2
    assert len(used) - E + F == 2, (len(used), E, F)
    # orientation: the fp64 normal against (centroid - centre); no triangle is small enough to be left out
    A, B, C = xyz64[tri[:, 0]], xyz64[tri[:, 1]], xyz64[tri[:, 2]]
    normal = np.cross(B - A, C - A)
    area = 0.5 * np.linalg.norm(normal, axis=1)
    assert area.min() >= 1e-6 * SPHERE_VOXEL ** 2, area.min()
    outward = (A + B + C) / 3 - np.array(SPHERE_C)
    assert ((normal * outward).sum(axis=1) > 0).all()
    # the distance to the sphere: linear interpolation of a function whose second derivative along an edge of length
    # at most L = sqrt(3) voxels is at most 1 / (R - L), plus the fp32 rounding of the coordinates
    L = np.sqrt(3.0) * SPHERE_VOXEL
    bound = L * L / (8 * (SPHERE_R - L)) + 4 * 2.0 ** -24 * np.abs(xyz64).max()
    err = np.abs(np.linalg.norm(xyz64 - np.array(SPHERE_C), axis=1) - SPHERE_R).max()
    assert err <= bound, (err, bound)
    return err, bound


# ---- checks shared by the two backends ----

def check_against(ref, xyz, rgb, tri, what):
    assert same_bits(xyz, ref["xyz"]), f"{what}: the vertices or their order differ"
    assert same_bits(rgb, ref["rgb"]), f"{what}: the colours differ"
    assert same_bits(tri, ref["tri"]), f"{what}: the triangles, their order or their orientation differ"


def check_capacity(mesh, fill_f, fill_b, fill_i):
    """with capacities 0, total - 1, total and total + 3, for the vertices and for the triangles independently, the rows
    below the capacity are the reference's and the rows at and past the count keep their fill"""
    ref = direct_reference()
    V, T = len(ref["xyz"]), len(ref["tri"])
    assert V > 40 and T > 40
    for vcap, tcap in [(c, T) for c in (0, V - 1, V, V + 3)] + [(V, c) for c in (0, T - 1, T + 3)]:
        xyz, rgb, tri = mesh(direct_planes(), DIRECT_ORIGIN, DIRECT_VOXEL, DIRECT_MIN_WEIGHT, vcap, tcap)
        assert xyz.shape == (vcap, 3) and rgb.shape == (vcap, 3) and tri.shape == (tcap, 3)
        nv, nt = min(vcap, V), min(tcap, T)
        assert same_bits(xyz[:nv], ref["xyz"][:nv]) and same_bits(rgb[:nv], ref["rgb"][:nv]), (vcap, tcap)
        assert same_bits(tri[:nt], ref["tri"][:nt]), (vcap, tcap)
        if fill_f is not None:
            assert np.isnan(xyz[nv:]).all() and (rgb[nv:] == fill_b).all() and (tri[nt:] == fill_i).all(), (vcap, tcap)
