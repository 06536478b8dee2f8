"""The cases tests/test_fusion_hostsim.py (host simulator) and tests/test_gpu_fusion.py (device) both run, each against
tests/fusion_oracle.py bit for bit: the five planes, the count, the points, their colours and their order.

A case is a volume and a list of integrate calls; `check(case, backend)` runs it through `backend.volume(...)` -- an
object with scsfm_hip.fusion.Volume's integrate / count / extract and a `planes` array -- once with all frames of a call in
one launch and once with one frame per launch, and through the oracle once (cached: the reference is computed once and
shared).  Frames are 12 x 20, the volume is 37 x 18 x 29 (no size a multiple of the 32 x 8 x 4 tile or of 4), 40 x 18 x 29
for the 16-byte path, 130 x 3 x 5 for rows that cross the waves and the 1024-voxel chunk of the extraction.
Test infrastructure only."""
from __future__ import annotations

import functools

import numpy as np

import fusion_oracle as O

H, W = 12, 20
K = np.array([[12.0, 0, 9.5], [0, 12.0, 5.5], [0, 0, 1]], np.float32)
DIMS = (37, 18, 29)
VOXEL = 0.1
ORIGIN = (-1.85, -0.9, 0.45)   # the volume spans x -1.85 .. 1.85, y -0.9 .. 0.9, z 0.45 .. 3.35
PLANE_Z = 2.03                 # the scene: the world plane z = PLANE_Z


def pose(yaw=0.0, pitch=0.0, pos=(0.0, 0.0, 0.0), skew=0.0):
    """camera-to-world [3, 4] float64: yaw about y, then pitch about x; `skew` leaves the rotation off orthonormal (the
    general inverse is what the library forms)"""
    cy, sy, cp, sp = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch)
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rx = np.array([[1, 0, 0], [0, cp, -sp], [0, sp, cp]])
    R = Ry @ Rx
    R = R + skew * np.array([[0.3, -1.0, 0.2], [0.7, 0.1, -0.4], [-0.6, 0.5, 0.9]])
    return np.concatenate([R, np.asarray(pos, np.float64)[:, None]], axis=1)


def render_plane(c2w, z0=PLANE_Z, noise=None):
    """the depth [H, W] float32 of the world plane z = z0 from the camera (0 where the ray does not meet it)"""
    px, py = np.meshgrid(np.arange(W), np.arange(H))
    rays = np.stack([(px - K[0, 2]) / K[0, 0], (py - K[1, 2]) / K[1, 1], np.ones_like(px, float)], -1)
    dz = rays @ c2w[2, :3]
    with np.errstate(all="ignore"):
        d = np.where(dz > 1e-6, (z0 - c2w[2, 3]) / dz, 0.0)
    d = np.where(d > 0, d, 0.0)
    if noise is not None:
        d = d * (1 + 0.01 * noise.standard_normal(d.shape))
    return d.astype(np.float32)


def _call(poses, rng, images=True, is_disp=False, near=0.05, max_depth=4.0, edit=None):
    c2w = np.stack(poses)
    depth = np.stack([render_plane(p, noise=rng) for p in c2w])
    if edit is not None:
        edit(depth)
    if is_disp:
        with np.errstate(all="ignore"):
            depth = np.where(depth > 0, np.float32(1) / depth, np.float32(0.01)).astype(np.float32)
    img = rng.standard_normal((len(c2w), 3, H, W)).astype(np.float32) if images else None
    return dict(depth=depth, images=img, c2w=c2w, K=K, is_disp=is_disp, near=near, max_depth=max_depth)


def _straddle(n, rng):
    """n cameras outside the volume, turned so that each of a frustum's four planes and the near / far range cuts
    through tiles"""
    views = [(0.6, 0.0, (-1.6, 0.0, 0.2)), (-0.6, 0.0, (1.6, 0.1, 0.2)), (0.0, 0.45, (0.2, -0.9, 0.1)),
             (0.0, -0.45, (-0.2, 0.9, 0.1)), (0.3, 0.2, (-0.5, -0.3, 0.0)), (-0.25, -0.15, (0.4, 0.2, -0.2)),
             (0.9, 0.1, (-2.2, 0.0, 1.0)), (-0.8, -0.1, (2.0, 0.0, 0.9))]
    return [pose(y, p, t, skew=1e-7 * (i % 3)) for i, (y, p, t) in enumerate(views[:n])]


def _dirty(depth):
    depth[0, 2:5, 3:9] = 0.0
    depth[0, 6:8, 10:15] = np.nan
    depth[1, :, :4] = 7.5          # above max_depth
    depth[1, 9:, 12:] = np.inf
    depth[2, 3:6, 5:11] = -1.0


def _dirty_disp(depth):
    depth[0, 2:5, 3:9] = 0.0       # -> the minimum disparity 0.01 (a depth of 100, above max_depth)
    depth[1, 6:8, 10:15] = np.nan
    depth[2, 1:3, :] = 1e-30       # a disparity whose reciprocal overflows


@functools.lru_cache(maxsize=None)
def cases():
    rng = np.random.default_rng(20)
    out = {}

    def add(name, calls, dims=DIMS, origin=ORIGIN, voxel=VOXEL, trunc=None, max_weight=64.0, planes=None, min_weight=1.0):
        out[name] = dict(name=name, dims=dims, origin=origin, voxel=voxel, trunc=trunc, max_weight=max_weight,
                         calls=calls, planes=planes, min_weight=min_weight)

    add("straddle_F5", [_call(_straddle(5, rng), rng)])
    add("straddle_F8_vec", [_call(_straddle(8, rng), rng)], dims=(40, 18, 29))
    add("F1", [_call(_straddle(1, rng), rng)])
    add("inside", [_call([pose(0.2, 0.1, (0.1, 0.05, 1.1)), pose(-2.8, 0.0, (0.0, 0.0, 2.9))], rng)])
    add("dirty_depth", [_call(_straddle(5, rng), rng, edit=_dirty)])
    add("dirty_disp", [_call(_straddle(5, rng), rng, is_disp=True, edit=_dirty_disp)])
    add("max_weight", [_call(_straddle(8, rng)[4:6] * 4, rng)], max_weight=3.0)
    add("no_image", [_call(_straddle(5, rng), rng), _call(_straddle(8, rng)[3:], rng, images=False)])
    add("no_image_alone", [_call(_straddle(5, rng), rng, images=False)])
    add("min_weight_2", [_call(_straddle(8, rng), rng)], min_weight=2.0)
    add("chunk_x", [_call([pose(0.0, 0.0, (0.0, 0.0, 0.0)), pose(0.3, 0.0, (-2.0, 0.0, 0.2)),
                           pose(-0.3, 0.0, (2.0, 0.0, 0.2))], rng)],
        dims=(130, 3, 5), origin=(-6.5, -0.15, 1.78), trunc=0.25)
    add("empty", [])
    # planes set by hand: a voxel with tsdf exactly 0.0 and one with -0.0 between neighbours of either sign (neither is
    # "< 0", so each crosses only towards a negative neighbour), unseen voxels and a weight below min_weight
    nx, ny, nz = 9, 4, 3
    planes = np.zeros((5, nz, ny, nx), np.float32)
    planes[0] = rng.uniform(-1, 1, (nz, ny, nx)).astype(np.float32)
    planes[1] = rng.integers(0, 4, (nz, ny, nx)).astype(np.float32)
    planes[2:] = rng.uniform(-0.1, 1.1, (3, nz, ny, nx)).astype(np.float32)
    planes[0, 1, 1, 2], planes[0, 1, 2, 5] = 0.0, -0.0
    planes[0, 1, 1, 1], planes[0, 1, 1, 3], planes[0, 1, 2, 4], planes[0, 1, 2, 6] = -0.4, 0.3, -0.2, 0.6
    planes[1, 1, 1, 1:4] = planes[1, 1, 2, 4:7] = 2
    add("signed_zeros", [], dims=(nx, ny, nz), origin=(0.0, 0.0, 0.0), planes=planes, min_weight=2.0)
    return out


NAMES = ("straddle_F5", "straddle_F8_vec", "F1", "inside", "dirty_depth", "dirty_disp", "max_weight", "no_image",
         "no_image_alone", "min_weight_2", "chunk_x", "empty", "signed_zeros")


@functools.lru_cache(maxsize=None)
def reference(name):
    """the oracle's volume of the case (computed once; read-only afterwards)"""
    case = cases()[name]
    vol = O.Volume(case["dims"], case["origin"], case["voxel"], case["trunc"], case["max_weight"])
    if case["planes"] is not None:
        vol.planes[...] = case["planes"]
    for call in case["calls"]:
        vol.integrate(**call)
    xyz, rgb, axis = vol.extract(case["min_weight"])
    for a in (vol.planes, xyz, rgb, axis):
        a.setflags(write=False)
    return vol, xyz, rgb, axis


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def run(case, backend, frames_per_launch):
    vol = backend.volume(case["dims"], case["origin"], case["voxel"], case["trunc"], case["max_weight"], frames_per_launch)
    if case["planes"] is not None:
        backend.set_planes(vol, case["planes"])
    for call in case["calls"]:
        vol.integrate(backend.dev(call["depth"]), None if call["images"] is None else backend.dev(call["images"]),
                      backend.dev(call["c2w"]), backend.dev(call["K"]), is_disp=call["is_disp"], near=call["near"],
                      max_depth=call["max_depth"])
    return vol


def check(name, backend):
    """the case against the oracle, bit for bit: with all frames of a call in one launch, and one frame per launch"""
    case = cases()[name]
    ref, xyz, rgb, _ = reference(name)
    most = max([len(c["depth"]) for c in case["calls"]] + [1])
    for fpl in sorted({most, 1}):
        vol = run(case, backend, fpl)
        planes = backend.host(vol.planes)
        for k, plane in enumerate(("tsdf", "weight", "r", "g", "b")):
            assert same_bits(planes[k], ref.planes[k]), f"{name}: the {plane} plane differs at {fpl} frames per launch"
        n, ws = vol.count(case["min_weight"])
        ws = backend.host(ws)
        nc = len(ref.chunk_counts(case["min_weight"]))
        assert n == len(xyz) and ws[0] == n, (name, n, len(xyz))
        assert np.array_equal(ws[4:4 + nc], ref.chunk_counts(case["min_weight"])), name
        assert np.array_equal(ws[4 + nc:4 + 2 * nc], np.cumsum(ws[4:4 + nc]) - ws[4:4 + nc]), name
        got_xyz, got_rgb = (backend.host(a) for a in vol.extract(case["min_weight"]))
        assert same_bits(got_xyz, xyz), f"{name}: the points or their order differ"
        assert same_bits(got_rgb, rgb), f"{name}: the colours differ"
    return vol, n


def check_capacity(name, backend):
    """a capacity below the count writes the first rows and nothing at or past it; one equal to it writes all"""
    case = cases()[name]
    _, xyz, rgb, _ = reference(name)
    n = len(xyz)
    assert n > 40
    vol = run(case, backend, 8)
    for cap in (n, n - 37, 1):
        got_xyz, got_rgb = backend.extract_guarded(vol, case["min_weight"], cap)
        assert same_bits(got_xyz, xyz[:cap]) and same_bits(got_rgb, rgb[:cap]), (name, cap)


# ---- the analytic case ----

D0 = 1.73
ANALYTIC = dict(dims=(24, 14, 22), origin=(-1.2, -0.7, 0.4), voxel_size=0.1, trunc=0.3)


def analytic_call():
    """a fronto-parallel plane at depth D0 seen by three cameras with identity rotation, translated sideways"""
    c2w = np.stack([pose(pos=(x, 0.0, 0.0)) for x in (-0.4, 0.0, 0.4)])
    depth = np.full((3, H, W), D0, np.float32)
    return dict(depth=depth, images=None, c2w=c2w, K=K, is_disp=False, near=0.05, max_depth=4.0)


def analytic_columns():
    """[ny, nx] bool: the columns of voxels whose point at depth D0 some camera sees (its pixel inside the picture)"""
    call, (nx, ny, _) = analytic_call(), ANALYTIC["dims"]
    x = ANALYTIC["origin"][0] + (np.arange(nx) + 0.5) * ANALYTIC["voxel_size"]
    y = ANALYTIC["origin"][1] + (np.arange(ny) + 0.5) * ANALYTIC["voxel_size"]
    seen = np.zeros((ny, nx), bool)
    for p in call["c2w"]:
        u = K[0, 0] * (x[None, :] - p[0, 3]) / D0 + K[0, 2]
        v = K[1, 1] * (y[:, None] - p[1, 3]) / D0 + K[1, 2]
        seen |= (u >= 0) & (u <= W - 1) & (v >= 0) & (v <= H - 1)  # (the pixel's centre, not its border: strictly inside)
    return seen


@functools.lru_cache(maxsize=1)
def analytic_reference():
    vol = O.Volume(**ANALYTIC)
    vol.integrate(**analytic_call())
    xyz, rgb, axis = vol.extract(1.0)
    return vol, xyz, rgb, axis


def plane_statistics(xyz, axis):
    """-> (the largest |z - D0| over the points of z-edges, the share of the in-frustum columns with such a point)"""
    pts = xyz[axis == 2]
    nx, ny, _ = ANALYTIC["dims"]
    ix = np.floor((pts[:, 0] - ANALYTIC["origin"][0]) / ANALYTIC["voxel_size"]).astype(int)
    iy = np.floor((pts[:, 1] - ANALYTIC["origin"][1]) / ANALYTIC["voxel_size"]).astype(int)
    hit = np.zeros((ny, nx), bool)
    hit[iy, ix] = True
    cols = analytic_columns()
    return float(np.abs(pts[:, 2].astype(np.float64) - D0).max()), float((hit & cols).sum() / cols.sum())
