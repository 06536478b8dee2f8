"""The cases tests/test_raycast_hostsim.py (host simulator) and tests/test_gpu_raycast.py (device) both run, each against
tests/raycast_oracle.py bit for bit on all four outputs.

A case is a volume (the five planes), view records and a march; `check(name, backend)` casts it through
`backend.cast(planes, origin, voxel, view, hw, near, step, n_steps, min_weight, mask, normals, colour, shade)` -- which
returns a dict of numpy arrays -- with the backend's brick mask, with no mask and with a mask of all ones, and compares
the mask itself with the oracle's.  The volume is 40 x 18 x 29 (no size a multiple of the 8-voxel brick: the last bricks are
clipped), the views are 12 x 20 (the 16 x 16 pixel tiles are partial), at most three a call.  The references are computed
once (cached) and read-only.

So that no case passes by having no hits, `reference` asserts on the oracle alone that every view meant to hit (a case's
`hits`) has a hit in at least half of its pixels, and that the views meant to end on the back-face rule (`backs`) have
no hit and at least one ray ended by that rule.  Test infrastructure only."""
from __future__ import annotations

import functools

import numpy as np

import fusion_oracle as FO
import raycast_oracle as RO
from _fusion_cases import H, K, ORIGIN, VOXEL, W, pose, same_bits

f32 = np.float32
HW = (H, W)
DIMS = (40, 18, 29)            # x -1.85 .. 2.15, y -0.9 .. 0.9, z 0.45 .. 3.35
TRUNC = 3 * VOXEL
PLANE_D = 1.73                 # the fused scene: the world plane z = PLANE_D
PLANE_X = (-0.5, 0.0, 0.5)     # the fusing cameras: identity rotation, at (x, 0, 0)
SPHERE_C = (0.15, 0.02, 1.9)
SPHERE_R = 0.5
WALL_Z = 2.9                   # the solid z > WALL_Z behind the sphere
K_CENTRED = np.array([[12.0, 0, 9.0], [0, 12.0, 5.0], [0, 0, 1]], np.float32)    # pixel (9, 5) looks along the axis
K_TELE = np.array([[30.0, 0, 9.5], [0, 30.0, 5.5], [0, 0, 1]], np.float32)       # a view that stays inside the box
K_NARROW = np.array([[200.0, 0, 9.5], [0, 200.0, 5.5], [0, 0, 1]], np.float32)
KEYS = ("depth", "normal", "rgb", "shade")


@functools.lru_cache(maxsize=1)
def plane_planes():
    """a fronto-parallel plane at depth PLANE_D fused by the fusion oracle from three cameras, with random images"""
    rng = np.random.default_rng(7)
    vol = FO.Volume(DIMS, ORIGIN, VOXEL)
    c2w = np.stack([pose(pos=(x, 0.0, 0.0)) for x in PLANE_X])
    depth = np.full((3, H, W), PLANE_D, np.float32)
    images = rng.standard_normal((3, 3, H, W)).astype(np.float32)
    vol.integrate(depth, images, c2w, K, is_disp=False, near=0.05, max_depth=4.0)
    vol.planes.setflags(write=False)
    return vol.planes


def _centres(dims=DIMS, origin=ORIGIN, voxel=VOXEL):
    nx, ny, nz = dims
    x = FO.centres(origin[0], nx, voxel)[None, None, :]
    y = FO.centres(origin[1], ny, voxel)[None, :, None]
    z = FO.centres(origin[2], nz, voxel)[:, None, None]
    return x, y, z


@functools.lru_cache(maxsize=None)
def sphere_planes(wall=False, dims=DIMS):
    """t = clip((|p - c| - R) / trunc, -1, 1) in fp32 at the voxel centres, with `wall` the union with the solid
    z > WALL_Z; weight 1 everywhere; colours that vary with the place, a little outside [0, 1]"""
    x, y, z = _centres(dims)
    cx, cy, cz = (f32(v) for v in SPHERE_C)
    d = np.sqrt((x - cx) * (x - cx) + (y - cy) * (y - cy) + (z - cz) * (z - cz)) - f32(SPHERE_R)
    if wall:
        d = np.minimum(d, f32(WALL_Z) - z + 0 * x + 0 * y)
    nx, ny, nz = dims
    planes = np.zeros((5, nz, ny, nx), np.float32)
    planes[0] = np.clip(d / f32(TRUNC), f32(-1), f32(1))
    planes[1] = 1
    planes[2] = 0.5 + 0.6 * np.sin(3 * x) + 0 * y + 0 * z
    planes[3] = 0.5 + 0.6 * np.cos(4 * y) + 0 * x + 0 * z
    planes[4] = 0.5 + 0.3 * np.sin(5 * z) + 0 * x + 0 * y
    planes.setflags(write=False)
    return planes


def _gap_planes():
    planes = plane_planes().copy()
    planes[1, 5:7] = 0.5              # a slab between the cameras and the surface, below min_weight
    planes[1, :, :, 18:20] = 0.0      # and one that cuts the surface's band
    return planes


def _weights_1_3():
    planes = plane_planes().copy()
    seen = planes[1] > 0
    planes[1] = np.where(seen, 1.0, 0.0)
    planes[1, :, :, :26] = np.where(seen[:, :, :26], 3.0, 0.0)
    return planes


def _cell_planes():
    """2 x 2 x 2: one cell, its z = 0 face in free space and its z = 1 face inside"""
    planes = np.zeros((5, 2, 2, 2), np.float32)
    planes[0, 0], planes[0, 1] = [[0.6, 0.5], [0.7, 0.4]], [[-0.5, -0.6], [-0.3, -0.8]]
    planes[1] = 2
    planes[2:] = np.linspace(0.1, 0.9, 24, dtype=np.float32).reshape(3, 2, 2, 2)
    return planes


def _records(poses, Ks):
    """view records of poses with an intrinsic matrix each"""
    return np.concatenate([RO.views(p[None], k) for p, k in zip(poses, Ks)])


@functools.lru_cache(maxsize=1)
def cases():
    out = {}

    def add(name, planes, poses, Ks=None, origin=ORIGIN, voxel=VOXEL, near=0.0, step=VOXEL, n_steps=30, min_weight=1.0,
            hits=(), backs=(), edit=None):
        poses = list(poses)
        view = _records(poses, Ks or [K] * len(poses))
        if edit is not None:
            edit(view)
        assert len(view) <= 3
        planes = np.ascontiguousarray(planes, np.float32)
        planes.setflags(write=False)
        view.setflags(write=False)
        out[name] = dict(name=name, planes=planes, origin=origin, voxel=voxel, view=view, hw=HW, near=near, step=step,
                         n_steps=n_steps, min_weight=min_weight, hits=tuple(hits), backs=tuple(backs))

    fusing = pose(pos=(0.0, 0.0, 0.0))
    turned = pose(0.25, -0.15, (0.3, 0.1, 0.2))
    outside = pose(pos=(SPHERE_C[0], SPHERE_C[1], 1.0))
    centre = pose(0.1, 0.05, SPHERE_C)
    add("plane", plane_planes(), [fusing, turned], hits=(0, 1))
    add("sphere_outside", sphere_planes(), [outside, pose(0.2, 0.1, (0.0, -0.05, 1.05))], hits=(0,))
    add("sphere_inside", sphere_planes(), [centre], backs=(0,))
    add("behind_back_face", sphere_planes(True), [centre, outside], hits=(1,), backs=(0,))
    add("empty", np.zeros((5, DIMS[2], DIMS[1], DIMS[0]), np.float32), [fusing, turned])
    add("unseen_gap", _gap_planes(), [fusing, turned], hits=(0,))
    add("outside_box", sphere_planes(True), [pose(pos=(0.1, 0.0, -0.5)), pose(pos=(5.0, 0.0, 0.0)),
                                             pose(np.pi, 0.0, (0.0, 0.0, 0.2))], Ks=[K_TELE, K, K], n_steps=40, hits=(0,))

    def spoil(view):
        view[1, 10] = np.nan
        view[2, 9] = 1e30
    add("axis_nan_huge", sphere_planes(True), [pose(pos=(0.0, 0.0, 0.6))] * 3, Ks=[K_CENTRED] * 3, hits=(0,), edit=spoil)
    add("thin_x", sphere_planes(True, (1, 18, 29)), [fusing, outside])
    add("one_cell", _cell_planes(), [pose(pos=(0.1, 0.1, 0.9))], Ks=[K_NARROW], origin=(0.0, 0.0, 1.0), step=0.02,
        n_steps=20, min_weight=2.0, hits=(0,))
    add("one_step", plane_planes(), [fusing], near=1.7, n_steps=1)
    add("two_steps", plane_planes(), [fusing], near=1.7, n_steps=2, hits=(0,))
    add("long_step_near", plane_planes(), [fusing, turned], near=0.35, step=2.5 * VOXEL, n_steps=12, hits=(0,))
    add("min_weight_2", _weights_1_3(), [fusing, turned], min_weight=2.0, hits=(0,))
    return out


NAMES = ("plane", "sphere_outside", "sphere_inside", "behind_back_face", "empty", "unseen_gap", "outside_box",
         "axis_nan_huge", "thin_x", "one_cell", "one_step", "two_steps", "long_step_near", "min_weight_2")
BATCHED = "outside_box"    # three views: one call equals three calls of one
NULLS = "plane"


def _oracle(case, view=None):
    return RO.cast(case["planes"], case["origin"], case["voxel"], case["view"] if view is None else view, case["hw"],
                   case["near"], case["step"], case["n_steps"], case["min_weight"])


@functools.lru_cache(maxsize=None)
def reference(name):
    """the oracle's outputs and brick mask of the case (computed once; read-only afterwards), with the conditions on the
    case itself: enough hits where hits are meant, the back-face rule where it is meant"""
    case = cases()[name]
    ref = _oracle(case)
    ref["mask"] = RO.brick_mask(case["planes"], case["min_weight"])
    for v in case["hits"]:
        assert ref["hit"][v].mean() >= 0.5, (name, v, ref["hit"][v].mean())
    for v in case["backs"]:
        assert not ref["hit"][v].any() and ref["back"][v].any(), (name, v)
    for a in ref.values():
        a.setflags(write=False)
    return ref


def _cast(case, backend, view=None, mask=None, normals=True, colour=True, shade=True):
    return backend.cast(case["planes"], case["origin"], case["voxel"], case["view"] if view is None else view,
                        case["hw"], case["near"], case["step"], case["n_steps"], case["min_weight"], mask, normals,
                        colour, shade)


def compare(got, ref, what, views=slice(None)):
    for key in KEYS:
        if got[key] is not None:
            assert same_bits(got[key], ref[key][views]), f"{what}: {key} differs"


def check(name, backend):
    """the case against the oracle, bit for bit: with the backend's brick mask (itself the oracle's, byte for byte), with
    no mask and with a mask of all ones"""
    case, ref = cases()[name], reference(name)
    mask = backend.brick_mask(case["planes"], case["min_weight"])
    assert same_bits(mask, ref["mask"]), f"{name}: the brick mask differs"
    for label, m in (("culled", mask), ("mask == NULL", None), ("a mask of ones", np.ones_like(mask))):
        compare(_cast(case, backend, mask=m), ref, f"{name}, {label}")
    return ref


def check_batches(backend, name=BATCHED):
    """V views in one call equal V calls of one view"""
    case, ref = cases()[name], reference(name)
    mask = backend.brick_mask(case["planes"], case["min_weight"])
    assert len(case["view"]) == 3
    for v in range(3):
        compare(_cast(case, backend, view=case["view"][v:v + 1], mask=mask), ref, f"{name}, view {v} alone",
                slice(v, v + 1))


def check_null_outputs(backend, name=NULLS):
    """each optional output NULL in turn, and all three: the others are the same bits"""
    case, ref = cases()[name], reference(name)
    mask = backend.brick_mask(case["planes"], case["min_weight"])
    for normals, colour, shade in ((False, True, True), (True, False, True), (True, True, False), (False, False, False)):
        got = _cast(case, backend, mask=mask, normals=normals, colour=colour, shade=shade)
        assert (got["normal"] is None) == (not normals) and (got["rgb"] is None) == (not colour)
        assert (got["shade"] is None) == (not shade) and got["depth"] is not None
        compare(got, ref, f"{name}, normals={normals} colour={colour} shade={shade}")


# ---- analytic checks, on the oracle ----

def plane_depth_error():
    """the largest |depth - the ray's true depth to the plane| over the hits of the "plane" case's two views; the true
    depth along a ray with camera-frame z = 1 is (PLANE_D - c_z) / w_z"""
    case, ref = cases()["plane"], reference("plane")
    c, w = RO.rays(case["view"], case["hw"])
    true = (PLANE_D - c[2].astype(np.float64)) / w[2].astype(np.float64)
    err = np.abs(ref["depth"].astype(np.float64) - true)[ref["hit"]]
    return float(err.max())


def plane_central_shade():
    """the shade bytes of the central 4 x 6 pixels of the fusing view: the plane faces the camera, so L is cos of the
    ray's angle to the axis"""
    ref = reference("plane")
    return ref["shade"][0, 4:8, 7:13]


def sphere_errors():
    """over the hits ON THE SPHERE of "sphere_outside"'s first view: the largest |depth - ray-sphere intersection| and the
    largest angle (radians) between the normal and the radial direction"""
    case, ref = cases()["sphere_outside"], reference("sphere_outside")
    c, w = RO.rays(case["view"][:1], case["hw"])
    o = np.stack([np.broadcast_to(ci.astype(np.float64), w[0].shape) for ci in c], -1) - np.array(SPHERE_C)
    d = np.stack([wi.astype(np.float64) for wi in w], -1)
    a, b, cc = (d * d).sum(-1), 2 * (o * d).sum(-1), (o * o).sum(-1) - SPHERE_R ** 2
    disc = b * b - 4 * a * cc
    hit = ref["hit"][:1]
    assert (disc[hit] > 0).all()
    with np.errstate(all="ignore"):
        s = (-b - np.sqrt(disc)) / (2 * a)
    depth_err = np.abs(ref["depth"][:1].astype(np.float64) - s)[hit].max()
    p = o + s[..., None] * d
    radial = p / np.linalg.norm(p, axis=-1, keepdims=True)
    n = np.moveaxis(ref["normal"][:1].astype(np.float64), 1, -1)
    cos = np.clip((n * radial).sum(-1), -1, 1)[hit]
    return float(depth_err), float(np.arccos(cos).max())
