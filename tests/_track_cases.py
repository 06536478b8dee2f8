"""The cases tests/test_tracking_hostsim.py (host simulator) and tests/test_gpu_tracking.py (device) both run, each against
tests/track_oracle.py bit for bit: the final states, their fp32 records, the c2w, every report row and the last
iteration's slab of partial sums.

A case is what `backend.align(depth, guess, K, ref_view, model_depth, model_normal, is_disp, near, max_depth, iterations,
max_dist, min_pairs)` takes -- it returns a dict of numpy arrays (state, est, c2w, report, slab).  The model maps come from
tests/raycast_oracle.py's cast of analytic volumes built as tests/_raycast_cases.py builds its sphere, from three
reference poses; the frames' depths from the same cast at three true poses; a call always carries V = 3 frames with
different guesses and different reference views.  The frames are 12 x 20 (one partial workgroup of 1024 pixels; 240 is no
multiple of the 256 threads) and 37 x 61 (2257 pixels: three workgroups, the last one partial with 209 pixels, no
multiple of the four pixels of a thread).  The references are computed once (cached) and read-only.

So that no case passes by being empty, `reference` asserts on the oracle alone that every frame of a case meant to
converge pairs at least half of its pixels in every iteration with a smallest pivot ratio of at least 1000 times the
header's SCSFM_TRACK_PIVOT_EPS, and that the degenerate frames report their status at iteration 0.  Test infrastructure
only."""
from __future__ import annotations

import functools

import numpy as np

import raycast_oracle as RO
import track_oracle as TO
from _fusion_cases import H, K, ORIGIN, VOXEL, W, pose, same_bits
from _raycast_cases import DIMS, SPHERE_C, SPHERE_R, TRUNC, _centres, plane_planes

f32 = np.float32
HW = (H, W)
HW_ODD = (37, 61)
K_ODD = np.array([[37.0, 0, 29.5], [0, 37.0, 17.5], [0, 0, 1]], np.float32)
N_STEPS = 40                    # the casts march to a depth of 4
MAX_DEPTH = 4.0
KEYS = ("state", "est", "c2w", "report", "slab")
# the room: the solid behind three mutually non-parallel planes, each (unit normal towards free space, offset)
ROOM = (((-0.15, 0.0, -1.0), 2.9), ((0.0, -1.0, -0.1), 0.75), ((-1.0, -0.1, 0.0), 1.2))
# (yaw, pitch, position): the true poses look into the room's corner; the reference poses are near them
TRUE = ((0.35, -0.20, (-0.30, -0.10, 0.50)), (0.30, -0.15, (-0.20, -0.05, 0.45)), (0.42, -0.22, (-0.35, -0.12, 0.55)))
REFS = ((0.33, -0.18, (-0.25, -0.08, 0.48)), (0.36, -0.19, (-0.28, -0.10, 0.52)), (0.38, -0.20, (-0.30, -0.08, 0.50)))
# the perturbed guesses: off by about one voxel (0.1) and one degree (0.0175 rad)
OFF = ((0.012, -0.012, (0.06, -0.05, 0.06)), (-0.014, 0.010, (-0.05, 0.06, -0.06)), (0.010, 0.014, (0.07, 0.04, -0.05)))


@functools.lru_cache(maxsize=1)
def room_planes():
    """t = clip(min(|p - c| - R, the three planes' distances) / trunc, -1, 1) at the voxel centres: a sphere in the corner
    of a room, which constrains all six degrees of freedom; weight 1 everywhere"""
    x, y, z = (a.astype(np.float64) for a in _centres(DIMS))
    cx, cy, cz = SPHERE_C
    d = np.sqrt((x - cx) ** 2 + (y - cy) ** 2 + (z - cz) ** 2) - SPHERE_R
    for n, off in ROOM:
        n = np.array(n) / np.linalg.norm(n)
        d = np.minimum(d, n[0] * x + n[1] * y + n[2] * z + off)
    nx, ny, nz = DIMS
    planes = np.zeros((5, nz, ny, nx), np.float32)
    planes[0] = np.clip(d / TRUNC, -1, 1).astype(np.float32)
    planes[1] = 1
    planes.setflags(write=False)
    return planes


def _poses(specs, off=None):
    if off is None:
        return np.stack([pose(y, p, t) for y, p, t in specs])
    return np.stack([pose(y + dy, p + dp, np.add(t, dt)) for (y, p, t), (dy, dp, dt) in zip(specs, off)])


@functools.lru_cache(maxsize=None)
def maps(scene, odd, which):
    """the oracle's cast of the scene's volume from the three true ("true") or reference ("ref") poses -> (view records,
    depth [3, H, W], normal [3, 3, H, W]), read-only"""
    planes = room_planes() if scene == "room" else plane_planes()
    specs = TRUE if which == "true" else REFS
    if scene == "plane":   # the cameras that fused it look along z
        specs = tuple((0.0, 0.0, (x, 0.0, 0.0)) for x in ((-0.1, 0.0, 0.1) if which == "true" else (0.0, 0.05, -0.05)))
    view = RO.views(_poses(specs), K_ODD if odd else K)
    out = RO.cast(planes, ORIGIN, VOXEL, view, HW_ODD if odd else HW, 0.0, VOXEL, N_STEPS, 1.0)
    got = (view, out["depth"], out["normal"])
    for a in got:
        a.setflags(write=False)
    return got


@functools.lru_cache(maxsize=1)
def cases():
    out = {}

    def add(name, guess, scene="room", odd=False, iterations=4, is_disp=False, max_dist=3 * VOXEL, min_pairs=24,
            converge=(0, 1, 2), status0=(0, 0, 0), edit=None):
        ref_view, M, N = maps(scene, odd, "ref")
        _, depth, _ = maps(scene, odd, "true")
        depth, M, N = depth.copy(), M.copy(), N.copy()
        if is_disp:
            with np.errstate(all="ignore"):
                depth = np.where(depth > 0, f32(1) / depth, f32(0.01)).astype(np.float32)
        if edit is not None:
            edit(depth, M, N)
        case = dict(depth=depth, guess=np.ascontiguousarray(guess, np.float64), K=K_ODD if odd else K, ref_view=ref_view,
                    model_depth=M, model_normal=N, is_disp=is_disp, near=0.05, max_depth=MAX_DEPTH, iterations=iterations,
                    max_dist=max_dist, min_pairs=min_pairs)
        for a in case.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        out[name] = dict(name=name, args=case, converge=tuple(converge), status0=tuple(status0))

    truth, guess = _poses(TRUE), _poses(TRUE, OFF)
    add("truth", truth, iterations=1)
    add("perturbed", guess)
    add("perturbed_one_iteration", guess, iterations=1)
    add("perturbed_odd_size", guess, odd=True)

    def spoil(depth, M, N):
        depth[0, 2, 3], depth[0, 2, 4], depth[1, 5, 7], depth[2, 8, 11] = 0.01, 0.0, np.nan, 0.0
        depth[2, 0, 0] = np.nan
    add("disparity", guess, is_disp=True, edit=spoil)
    away = guess.copy()
    away[1] = pose(TRUE[1][0] + np.pi, 0.0, TRUE[1][2])
    add("looks_away", away, converge=(0, 2), status0=(0, 1, 0))
    add("plane_rank_deficient", _poses(((0.0, 0.0, (-0.1, 0.0, 0.0)), (0.01, 0.0, (0.0, 0.02, 0.03)), (0.0, -0.01, (0.12, 0.0, -0.03)))),
        scene="plane", converge=(), status0=(2, 2, 2))
    add("small_max_dist", guess, max_dist=0.09, converge=())

    def holes(depth, M, N):
        M[0, 3:7, 4:11], M[1, :, :3], M[2, 6, 6] = 0.0, np.nan, -1.0
        N[0, :, 8:10, 12:16], N[1, 1, 4, 4], N[2, :, 2:4, :] = 0.0, np.nan, 0.0
    add("holes", guess, converge=(), edit=holes)
    return out


NAMES = ("truth", "perturbed", "perturbed_one_iteration", "perturbed_odd_size", "disparity", "looks_away",
         "plane_rank_deficient", "small_max_dist", "holes")


@functools.lru_cache(maxsize=None)
def reference(name):
    """the oracle's result of the case (computed once; read-only afterwards), with the conditions on the case itself"""
    case = cases()[name]
    ref = TO.align(**case["args"])
    rep = ref["report"]
    n_pix = case["args"]["depth"][0].size
    for v in case["converge"]:
        assert (rep[v, :, 2] == 0).all(), (name, v, rep[v])
        assert rep[v, :, 0].min() >= 0.5 * n_pix, (name, v, rep[v, :, 0], n_pix)
        assert rep[v, :, 3].min() >= 1000 * TO.PIVOT_EPS, (name, v, rep[v, :, 3])
    state0, _ = TO.init(case["args"]["guess"], case["args"]["K"])
    for v, status in enumerate(case["status0"]):
        assert rep[v, 0, 2] == status, (name, v, rep[v])
        if status:   # a degenerate frame: every iteration the same, the state the same bits as the guess's
            assert (rep[v, :, 2] == status).all() and same_bits(ref["state"][v], state0[v]), (name, v)
        if status == 1:
            assert (rep[v, :, 0] < case["args"]["min_pairs"]).all()
    for a in ref.values():
        a.setflags(write=False)
    return ref


def pair_counts(name):
    """the pairs of iteration 0, per frame"""
    return reference(name)["report"][:, 0, 0]


def check(name, backend):
    """the case through `backend.align` against the oracle, bit for bit"""
    case, ref = cases()[name], reference(name)
    got = backend.align(**case["args"])
    for key in KEYS:
        assert got[key].shape == ref[key].shape and same_bits(got[key], ref[key]), f"{name}: {key} differs"
    return ref


# ---- convergence, on the oracle ----

def pose_errors(c2w, truth):
    """-> (translation errors [V], rotation angles [V] in radians) of c2w against truth"""
    c2w, truth = np.asarray(c2w, np.float64), np.asarray(truth, np.float64)
    dt = np.linalg.norm(c2w[:, :, 3] - truth[:, :, 3], axis=1)
    R = np.einsum("vij,vkj->vik", c2w[:, :, :3], truth[:, :, :3])
    ang = np.arccos(np.clip((np.trace(R, axis1=1, axis2=2) - 1) / 2, -1, 1))
    return dt, ang


@functools.lru_cache(maxsize=None)
def convergence(odd=True, iterations=10):
    """ten iterations of the oracle from the perturbed guesses on the room -> dict(gain_t, gain_r: the sum of the three
    frames' errors of the guesses over that of the estimates; rms [iterations]: sqrt(sum r^2 / count) summed over the
    frames' sums)"""
    args = dict(cases()["perturbed_odd_size" if odd else "perturbed"]["args"], iterations=iterations)
    ref = TO.align(**args)
    truth = _poses(TRUE)
    t0, r0 = pose_errors(args["guess"], truth)
    t1, r1 = pose_errors(ref["c2w"], truth)
    rep = ref["report"]
    assert (rep[:, :, 2] == 0).all()
    rms = np.sqrt(rep[:, :, 1].sum(0) / rep[:, :, 0].sum(0))
    return dict(gain_t=float(t0.sum() / t1.sum()), gain_r=float(r0.sum() / r1.sum()), rms=rms, t0=t0, t1=t1, r0=r0, r1=r1)
