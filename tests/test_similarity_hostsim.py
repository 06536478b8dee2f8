"""The 7-DoF tracking kernels of csrc_sim3/ on the host simulator against tests/sim3_oracle.py, bit for bit on the states,
their records, the fp32 scales, the poses, the scales, every report row and the slab of partial sums
(tests/_sim3_cases.py: the cases; the simulator's guard bands round every array are the guard rows); the cross-library
check against libscsfm_track's own host build; the streaming scale; and the convergence of the algorithm itself, judged
on the oracle."""
import numpy as np
import pytest

import _hostsim_sim3 as HS
import _hostsim_track as HT
import _sim3_cases as SC
import _track_cases as TC
import sim3_oracle as SO
import track_oracle as TO


class Backend:
    align = staticmethod(HS.align)


class TrackBackend:
    align = staticmethod(HT.align)


def test_the_cases_are_the_listed_ones():
    assert tuple(SC.cases()) == SC.NAMES
    assert (SO.TILE, SO.THREADS) == (TO.TILE, TO.THREADS) and SO.SUMS == 37 and len(SO.PAIRS) == 28
    sizes = set()
    for name, case in SC.cases().items():
        a = case["args"]
        V = 1 if name == "single_frame" else 3
        assert len(a["depth"]) == V and len({g.tobytes() for g in a["guess"]}) == V
        assert len({r.tobytes() for r in a["ref_view"]}) == V and a["scale0"].shape == (V,)
        sizes.add(a["depth"].shape[1:])
    assert sizes == {TC.HW, TC.HW_ODD}


@pytest.mark.parametrize("name", SC.NAMES)
def test_case_equals_the_oracle_bit_for_bit(name):
    SC.check(name, Backend)


@pytest.mark.parametrize("name", TC.NAMES)
def test_rigid_step_equals_the_track_library_bit_for_bit(name):
    """scale0 = 1 and min_scale_pivot = inf: the pose part of the state, the record, the c2w and the report's count, sum
    of r r and pose pivot ratio are libscsfm_track's own (its host build), status 0 there being 3 here"""
    want = SC.check_against_track(name, Backend, TrackBackend)
    assert TC.same_bits(want["report"], TC.reference(name)["report"])      # (and that library's are its oracle's)


def test_the_cases_are_what_they_are_meant_to_be():
    """on the oracle alone: the scales found, what held means, and that the first iteration of four is the one iteration of
    the one-iteration case"""
    full, cut, holes = (SC.reference(n)["report"][:, 0, 0] for n in ("perturbed", "small_max_dist", "holes"))
    print("pairs at iteration 0: perturbed", full, "small max_dist", cut, "holes", holes)
    assert (cut < full).all() and (holes < full).all() and (holes > 0.5 * full).all()
    assert TC.same_bits(SC.reference("perturbed")["report"][:, :1], SC.reference("perturbed_one_iteration")["report"])
    for name, want in (("perturbed", (1.05, 1.05, 1.05)), ("perturbed_odd_size", (1.05, 0.93, 1.0)),
                       ("disparity", (1.05, 0.93, 1.0)), ("scale0_start", (1.05, 1.05, 1.05))):
        scale = SC.reference(name)["scale"]
        print(name, scale)
        assert np.abs(scale - want).max() < 0.005, (name, scale)
    # the report's last column is the scale BEFORE each update: the start, then what the iterations made of it
    rep = SC.reference("scale0_start")["report"]
    assert (rep[:, 0, 5] == 1.05).all() and (np.abs(rep[:, 1:, 5] - 1.05) < 0.01).all()
    rep = SC.reference("perturbed")["report"]
    assert (rep[:, 0, 5] == 1.0).all() and (rep[:, 1, 5] != 1.0).all()
    # held: the scale pivot is reported all the same, and the same system gives the same ratio
    held, free = SC.reference("scale_never_solved")["report"], SC.reference("perturbed")["report"]
    assert TC.same_bits(held[:, 0, :2], free[:, 0, :2]) and TC.same_bits(held[:, 0, 3:], free[:, 0, 3:])
    assert (held[:, :, 5] == 1.0).all()
    # a frame may hold its scale in one iteration and solve it in the next
    status = SC.reference("small_max_dist")["report"][:, :, 2]
    print("small_max_dist: status", status.tolist())
    assert set(status.reshape(-1).tolist()) <= {0.0, 3.0}
    # a NaN scale reports a NaN scale
    assert np.isnan(SC.reference("bad_scale0")["report"][1, :, 5]).all()


def test_init_and_poses_equal_the_oracle():
    rng = np.random.default_rng(3)
    c2w = [TC.pose(0.3, -0.2, (1.0, 2.0, 3.0)), TC.pose(np.pi - 0.01, 0.0, (0, 0, 0)), TC.pose(0.0, np.pi - 0.02, (0, 1, 0)),
           TC.pose(np.pi - 0.3, np.pi - 0.2, (5, 0, 0)), TC.pose(0.1, 0.2, (0, 0, 0), skew=1e-3)]
    c2w += [np.concatenate([np.linalg.qr(rng.standard_normal((3, 3)))[0], rng.standard_normal((3, 1))], 1) for _ in range(8)]
    c2w = np.stack(c2w)
    scale0 = np.array([1.0, 1.05, 0.0, np.nan, -1.0, np.inf, 1e-50, 1e50, 0.1 + 0.2, 1 / 3, 2.0, 0.93, 1e-40])
    state, est, sigma_f = HS.init(c2w, scale0, TC.K)
    want_state, want_est, want_sigma = SO.init(c2w, scale0, TC.K)
    assert TC.same_bits(state, want_state) and TC.same_bits(est, want_est) and TC.same_bits(sigma_f, want_sigma)
    assert {int(np.argmax(np.abs(s[:4]))) for s in want_state} == {0, 1, 2, 3}
    track_state, track_est = HT.init(c2w, TC.K)
    assert TC.same_bits(state[:, :7], track_state) and TC.same_bits(est, track_est)
    assert sigma_f[6] == 0 and np.isinf(sigma_f[7]) and 0 < sigma_f[12] < 1.2e-38        # (a denormal is kept)
    got_c2w, got_scale = HS.poses(state)
    want_c2w, want_scale = SO.poses(want_state)
    assert TC.same_bits(got_c2w, want_c2w) and TC.same_bits(got_scale, want_scale) and TC.same_bits(got_scale, scale0)


def _awkward_depth(rng, shape):
    d = rng.uniform(0.2, 5.0, shape).astype(np.float32)
    flat = d.reshape(-1)
    flat[:6] = (np.nan, 0.0, -0.0, 1e-45, 3e-39, np.inf)      # (denormals: 1e-45 is the smallest, 3e-39 a larger one)
    flat[-3:] = (-2.0, 3e38, 1e-30)
    return d


@pytest.mark.parametrize("shape", [(3, 12, 20), (3, 37, 61), (1, 1, 1), (2, 1, 3), (1, 5, 13)])
def test_scale_equals_numpys_product_bit_for_bit(shape):
    """the 16-byte path, its scalar tail (V H W no multiple of 4), the scalar path of pointers off a 16-byte boundary, and
    frames whose boundary falls inside a group of four"""
    rng = np.random.default_rng(5)
    depth = _awkward_depth(rng, shape) if np.prod(shape) >= 9 else rng.uniform(0.2, 5.0, shape).astype(np.float32)
    sigma_f = np.array([1.05, 0.93, 1e-39][:shape[0]], np.float32)
    for is_disp in (False, True):
        want = SO.scaled_depth(depth, sigma_f, is_disp)
        with np.errstate(all="ignore"):
            plain = sigma_f[:, None, None] * ((np.float32(1) / depth) if is_disp else depth)
        assert TC.same_bits(want, plain)
        for offset in (0, 1, 2):
            assert TC.same_bits(HS.scaled_depth(depth, sigma_f, is_disp, offset), want), (is_disp, offset)


def test_scaled_depth_is_the_depth_the_tracker_saw():
    """tracking the scaled depth with a scale of 1 sees the same pixels: with the scale held, the same sums"""
    a = SC.cases()["scale0_start"]["args"]
    held = HS.align(**dict(a, iterations=1, min_scale_pivot=np.inf))
    depth = HS.scaled_depth(a["depth"], a["scale0"].astype(np.float32), a["is_disp"])
    again = HS.align(**dict(a, depth=depth, scale0=np.ones(3), iterations=1, min_scale_pivot=np.inf))
    assert TC.same_bits(held["slab"], again["slab"]) and TC.same_bits(held["state"][:, :7], again["state"][:, :7])


def test_frames_in_one_call_equal_frames_one_by_one():
    case, ref = SC.cases()["perturbed_odd_size"]["args"], SC.reference("perturbed_odd_size")
    for v in range(3):
        one = {k: (a[v:v + 1] if isinstance(a, np.ndarray) and a.shape != (3, 3) else a) for k, a in case.items()}
        got = HS.align(**one)
        for key in SC.KEYS:
            assert TC.same_bits(got[key], ref[key][v:v + 1]), (v, key)
    assert TC.same_bits(SC.reference("single_frame")["state"], ref["state"][1:2])


def test_convergence_on_the_oracle():
    """Ten iterations from the perturbed guesses (off by a voxel and a degree) on the sphere in the room's corner, the sum
    over the three frames, every frame's depth divided by 1.05 -- a scale error of 5 % -- and by 0.93.

    Measured on the oracles (printed below).  Frames of 37 x 61, depth / 1.05: the 6-DoF oracle leaves a summed
    translation error of 0.192 and a rotation error of 0.142 rad (worse than the guesses' 0.051); the 7-DoF oracle 0.0021
    and 0.0012, with scales of 1.0501 .. 1.0507.  Frames of 12 x 20: 0.190 and 0.142 against 0.0113 and 0.0061, scales
    1.0499 .. 1.0519.  On exact depth the 7-DoF errors are about twice the 6-DoF oracle's (0.0021 against 0.0011 in
    translation at 37 x 61): the price of the seventh unknown.  The 6-DoF oracle's error over the 7-DoF oracle's, in
    translation / rotation: 89.6 / 121.7 (37 x 61, / 1.05), 151.3 / 171.0 (37 x 61, / 0.93), 16.8 / 23.1 (12 x 20, / 1.05),
    29.2 / 31.5 (12 x 20, / 0.93).  Asserted: at 37 x 61 the translation error below a tenth of the 6-DoF oracle's on the
    same input; every other factor at half of what the oracle gives; every scale within 0.005 of the factor; on exact
    depth both errors within a factor 4 of the 6-DoF oracle's."""
    for odd, factor, gain_t, gain_r in ((True, 1.05, 10.0, 121.7 / 2), (True, 0.93, 10.0, 171.0 / 2),
                                        (False, 1.05, 16.8 / 2, 23.1 / 2), (False, 0.93, 29.2 / 2, 31.5 / 2)):
        c = SC.convergence(odd, factor)
        print(f"odd={odd} depth / {factor}: translation {c['t0']:.4f} -> 6-DoF {c['t6']:.4f}, 7-DoF {c['t7']:.4f}; "
              f"rotation {c['r0']:.4f} -> {c['r6']:.4f}, {c['r7']:.4f}; scales {c['scale']}; scale pivot ratio "
              f"{c['report'][:, :, 4].min():.3g} .. {c['report'][:, :, 4].max():.3g}")
        assert (c["report"][:, :, 2] == 0).all()
        assert c["t7"] < c["t6"] / gain_t and c["r7"] < c["r6"] / gain_r
        assert np.abs(c["scale"] - factor).max() < 0.005
    for odd in (True, False):
        c = SC.convergence(odd, 1.0)
        print(f"odd={odd} exact depth: translation 6-DoF {c['t6']:.4f}, 7-DoF {c['t7']:.4f}; rotation {c['r6']:.4f}, "
              f"{c['r7']:.4f}; scales {c['scale']}")
        assert c["t7"] < 4 * c["t6"] and c["r7"] < 4 * c["r6"] and np.abs(c["scale"] - 1).max() < 0.005
