"""The cases tests/test_similarity_hostsim.py (host simulator) and tests/test_gpu_similarity.py (device) both run, each
against tests/sim3_oracle.py bit for bit: the final states, their fp32 records, the fp32 scales, the c2w, the scales, every
report row and the last iteration's slab of partial sums.

A case is what `backend.align(depth, guess, scale0, K, ref_view, model_depth, model_normal, is_disp, near, max_depth,
iterations, max_dist, min_pairs, min_scale_pivot)` takes -- it returns a dict of numpy arrays (KEYS).  The maps are
tests/_track_cases.py's: the room with the sphere at 12 x 20 (one partial workgroup) and 37 x 61 (three workgroups, the
last one partial), three frames with different guesses and reference views; "single_frame" carries V = 1.  A frame whose
depth is "divided by f" is the true depth over f, so that the scale that repairs it is f.  The room of the three planes
alone ("walls") is cast here in the same way: there n . u and n . t are constant on each plane and the scale is not
observable.

So that no case passes by being empty, `reference` asserts on the oracle alone that every frame of a case meant to
converge pairs at least half of its pixels, has status 0 in every iteration and a scale pivot ratio of at least five times
the default min_scale_pivot; that the frames of the planes-only room have status 3 in every iteration and a scale pivot
ratio of at most half the default; and that the degenerate frames report their status in every iteration and keep the
bits of their state.  Test infrastructure only."""
from __future__ import annotations

import functools

import numpy as np

import raycast_oracle as RO
import sim3_oracle as SO
import track_oracle as TO
import _track_cases as TC
from _fusion_cases import K, ORIGIN, VOXEL, pose, same_bits
from _raycast_cases import DIMS, TRUNC, _centres

f32 = np.float32
KEYS = ("state", "est", "sigma_f", "c2w", "scale", "report", "slab")
INF = float("inf")


@functools.lru_cache(maxsize=1)
def wall_planes():
    """_track_cases.room_planes without the sphere: the solid behind the three planes, weight 1 everywhere"""
    x, y, z = (a.astype(np.float64) for a in _centres(DIMS))
    d = None
    for n, off in TC.ROOM:
        n = np.array(n) / np.linalg.norm(n)
        e = n[0] * x + n[1] * y + n[2] * z + off
        d = e if d is None else np.minimum(d, e)
    nx, ny, nz = DIMS
    planes = np.zeros((5, nz, ny, nx), np.float32)
    planes[0] = np.clip(d / TRUNC, -1, 1).astype(np.float32)
    planes[1] = 1
    planes.setflags(write=False)
    return planes


@functools.lru_cache(maxsize=None)
def wall_maps(odd, which):
    view = RO.views(TC._poses(TC.TRUE if which == "true" else TC.REFS), TC.K_ODD if odd else K)
    out = RO.cast(wall_planes(), ORIGIN, VOXEL, view, TC.HW_ODD if odd else TC.HW, 0.0, VOXEL, TC.N_STEPS, 1.0)
    got = (view, out["depth"], out["normal"])
    for a in got:
        a.setflags(write=False)
    return got


@functools.lru_cache(maxsize=1)
def cases():
    out = {}

    def add(name, guess, scene="room", odd=False, iterations=4, is_disp=False, max_dist=3 * VOXEL, min_pairs=24,
            factors=(1.0, 1.0, 1.0), scale0=(1.0, 1.0, 1.0), min_scale_pivot=SO.MIN_SCALE_PIVOT, converge=(0, 1, 2),
            status=(0, 0, 0), edit=None, frames=slice(None)):
        get = wall_maps if scene == "walls" else functools.partial(TC.maps, scene)
        ref_view, M, N = get(odd, "ref")
        _, depth, _ = get(odd, "true")
        depth, M, N = depth.copy(), M.copy(), N.copy()
        with np.errstate(all="ignore"):
            depth = (depth / np.array(factors, np.float32)[:, None, None]).astype(np.float32)
            if is_disp:
                depth = np.where(depth > 0, f32(1) / depth, f32(0.01)).astype(np.float32)
        if edit is not None:
            edit(depth, M, N)
        case = dict(depth=depth[frames], guess=np.ascontiguousarray(guess, np.float64)[frames],
                    scale0=np.array(scale0, np.float64)[frames], K=TC.K_ODD if odd else K, ref_view=ref_view[frames],
                    model_depth=M[frames], model_normal=N[frames], is_disp=is_disp, near=0.05, max_depth=TC.MAX_DEPTH,
                    iterations=iterations, max_dist=max_dist, min_pairs=min_pairs, min_scale_pivot=min_scale_pivot)
        for key, a in case.items():
            if isinstance(a, np.ndarray):
                case[key] = a = np.ascontiguousarray(a)
                a.setflags(write=False)
        out[name] = dict(name=name, args=case, converge=tuple(converge), status=tuple(status))

    truth, guess = TC._poses(TC.TRUE), TC._poses(TC.TRUE, TC.OFF)
    add("truth", truth, iterations=1)
    add("perturbed", guess, factors=(1.05, 1.05, 1.05))
    add("perturbed_odd_size", guess, odd=True, factors=(1.05, 0.93, 1.0))
    add("perturbed_one_iteration", guess, iterations=1, factors=(1.05, 1.05, 1.05))

    def spoil(depth, M, N):
        depth[0, 2, 3], depth[0, 2, 4], depth[1, 5, 7], depth[2, 8, 11] = 0.01, 0.0, np.nan, 0.0
        depth[2, 0, 0] = np.nan
    add("disparity", guess, is_disp=True, factors=(1.05, 0.93, 1.0), edit=spoil)
    add("scale0_start", guess, factors=(1.05, 1.05, 1.05), scale0=(1.05, 1.05, 1.05))
    away = guess.copy()
    away[1] = pose(TC.TRUE[1][0] + np.pi, 0.0, TC.TRUE[1][2])
    add("looks_away", away, factors=(1.05, 1.05, 1.05), converge=(0, 2), status=(0, 1, 0))
    add("plane_rank_deficient", TC.cases()["plane_rank_deficient"]["args"]["guess"], scene="plane", converge=(),
        status=(2, 2, 2))
    add("walls_scale_held", guess, scene="walls", odd=True, factors=(1.05, 0.93, 1.0), converge=(), status=(3, 3, 3))
    add("scale_never_solved", guess, factors=(1.05, 1.05, 1.05), min_scale_pivot=INF, converge=(), status=(3, 3, 3))
    add("small_max_dist", guess, factors=(1.05, 1.05, 1.05), max_dist=0.09, converge=(), status=())

    def holes(depth, M, N):
        M[0, 3:7, 4:11], M[1, :, :3], M[2, 6, 6] = 0.0, np.nan, -1.0
        N[0, :, 8:10, 12:16], N[1, 1, 4, 4], N[2, :, 2:4, :] = 0.0, np.nan, 0.0
    add("holes", guess, factors=(1.05, 1.05, 1.05), converge=(), status=(), edit=holes)
    add("bad_scale0", guess, scale0=(0.0, np.nan, -1.0), converge=(), status=(2, 2, 2))
    add("single_frame", guess, odd=True, factors=(1.05, 0.93, 1.0), frames=slice(1, 2), converge=(0,), status=(0,))
    return out


NAMES = ("truth", "perturbed", "perturbed_odd_size", "perturbed_one_iteration", "disparity", "scale0_start", "looks_away",
         "plane_rank_deficient", "walls_scale_held", "scale_never_solved", "small_max_dist", "holes", "bad_scale0",
         "single_frame")


@functools.lru_cache(maxsize=None)
def reference(name):
    """the oracle's result of the case (computed once; read-only afterwards), with the conditions on the case itself"""
    case = cases()[name]
    args = case["args"]
    ref = SO.align(**args)
    rep = ref["report"]
    n_pix = args["depth"][0].size
    for v in case["converge"]:
        assert (rep[v, :, 2] == 0).all(), (name, v, rep[v])
        assert rep[v, :, 0].min() >= 0.5 * n_pix, (name, v, rep[v, :, 0], n_pix)
        assert rep[v, :, 3].min() >= 1000 * SO.PIVOT_EPS, (name, v, rep[v, :, 3])
        assert rep[v, :, 4].min() >= 5 * SO.MIN_SCALE_PIVOT, (name, v, rep[v, :, 4])
    state0, _, sigma0 = SO.init(args["guess"], args["scale0"], args["K"])
    for v, status in enumerate(case["status"]):
        assert (rep[v, :, 2] == status).all(), (name, v, rep[v])
        if status in (1, 2):   # a degenerate frame: the state the same bits as the guess's
            assert same_bits(ref["state"][v], state0[v]) and same_bits(ref["sigma_f"][v], sigma0[v]), (name, v)
        if status == 1:
            assert (rep[v, :, 0] < args["min_pairs"]).all()
        if status == 3:        # the pose moved, the scale kept its bits
            assert same_bits(ref["state"][v, 7], state0[v, 7]) and same_bits(ref["sigma_f"][v], sigma0[v]), (name, v)
            assert not same_bits(ref["state"][v, :7], state0[v, :7]), (name, v)
            assert rep[v, :, 0].min() >= 0.5 * n_pix, (name, v, rep[v, :, 0])
    if name == "walls_scale_held":
        assert 0 < rep[:, :, 4].min() and rep[:, :, 4].max() <= SO.MIN_SCALE_PIVOT / 2, rep[:, :, 4]
    for a in ref.values():
        a.setflags(write=False)
    return ref


def check(name, backend):
    """the case through `backend.align` against the oracle, bit for bit"""
    case, ref = cases()[name], reference(name)
    got = backend.align(**case["args"])
    for key in KEYS:
        assert got[key].shape == ref[key].shape and same_bits(got[key], ref[key]), f"{name}: {key} differs"
    return ref


# ---- the cross-library check ----

def check_against_track(name, backend, track_backend):
    """With scale0 = 1 and min_scale_pivot = inf the 7-DoF library takes the rigid step: _track_cases' case `name` through
    `backend.align` equals libscsfm_track's own result (`track_backend.align`) bit for bit in the pose part of the state,
    the record, the c2w, the report's count, sum of r r and pose pivot ratio; a status of 0 there is a 3 here."""
    args = TC.cases()[name]["args"]
    want = track_backend.align(**args)
    V = len(args["depth"])
    got = backend.align(**dict(args, scale0=np.ones(V), min_pairs=max(7, args["min_pairs"]), min_scale_pivot=INF))
    assert same_bits(got["state"][:, :7], want["state"]), name
    assert same_bits(got["state"][:, 7], np.ones(V)) and same_bits(got["sigma_f"], np.ones(V, np.float32)), name
    assert same_bits(got["est"], want["est"]) and same_bits(got["c2w"], want["c2w"]), name
    for mine, theirs in ((0, 0), (1, 1), (3, 3)):
        assert same_bits(got["report"][:, :, mine], want["report"][:, :, theirs]), (name, mine)
    status = want["report"][:, :, 2]
    assert same_bits(got["report"][:, :, 2], np.where(status == 0, 3.0, status)), name
    assert same_bits(got["report"][:, :, 5], np.ones_like(status)), name
    return want


# ---- convergence, on the oracle ----

@functools.lru_cache(maxsize=None)
def convergence(odd=True, factor=1.05, iterations=10):
    """ten iterations of both oracles from the perturbed guesses on the room, every frame's depth divided by `factor` ->
    dict(t6, r6: the 6-DoF oracle's summed translation and rotation errors at the end; t7, r7: the 7-DoF oracle's; t0,
    r0: the guesses'; scale [3]; report)"""
    name = "perturbed_odd_size" if odd else "perturbed"
    args = dict(cases()[name]["args"], iterations=iterations)
    with np.errstate(all="ignore"):
        args["depth"] = (TC.cases()[name]["args"]["depth"] / f32(factor)).astype(np.float32)
    args["scale0"] = np.ones(3)
    ref = SO.align(**args)
    rigid = TO.align(**{k: v for k, v in args.items() if k not in ("scale0", "min_scale_pivot")})
    truth = TC._poses(TC.TRUE)
    t0, r0 = TC.pose_errors(args["guess"], truth)
    t6, r6 = TC.pose_errors(rigid["c2w"], truth)
    t7, r7 = TC.pose_errors(ref["c2w"], truth)
    return dict(t0=float(t0.sum()), r0=float(r0.sum()), t6=float(t6.sum()), r6=float(r6.sum()), t7=float(t7.sum()),
                r7=float(r7.sum()), scale=ref["scale"], report=ref["report"])
