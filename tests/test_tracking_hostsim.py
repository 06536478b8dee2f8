"""The tracking kernels of csrc_track/ on the host simulator against tests/track_oracle.py, bit for bit on the states, their
records, the poses, every report row and the slab of partial sums (tests/_track_cases.py: the cases; the simulator's guard
bands round every array are the guard rows), and the convergence of the algorithm itself, judged on the oracle."""
import numpy as np
import pytest

import _hostsim_track as HT
import _track_cases as TC
import track_oracle as TO


class Backend:
    align = staticmethod(HT.align)


def test_the_cases_are_the_listed_ones():
    assert tuple(TC.cases()) == TC.NAMES
    odd = TC.HW_ODD[0] * TC.HW_ODD[1]
    assert -(-odd // TO.TILE) >= 3 and odd % TO.TILE and odd % TO.THREADS and odd % 4
    assert TC.H * TC.W % TO.THREADS and TC.H * TC.W < TO.TILE
    for case in TC.cases().values():
        a = case["args"]
        assert len(a["depth"]) == 3 and len({g.tobytes() for g in a["guess"]}) == 3
        assert len({r.tobytes() for r in a["ref_view"]}) == 3


@pytest.mark.parametrize("name", TC.NAMES)
def test_case_equals_the_oracle_bit_for_bit(name):
    TC.check(name, Backend)


def test_the_cases_are_what_they_are_meant_to_be():
    """on the oracle alone: what max_dist cuts, what the holes cost, and that the first iteration of four is the one
    iteration of the one-iteration case"""
    full, cut, holes = (TC.pair_counts(n) for n in ("perturbed", "small_max_dist", "holes"))
    print("pairs at iteration 0: perturbed", full, "small max_dist", cut, "holes", holes)
    assert (cut >= 0.25 * full).all() and (cut <= 0.75 * full).all()
    assert (holes < full).all() and (holes > 0.5 * full).all()
    assert TC.same_bits(TC.reference("perturbed")["report"][:, :1], TC.reference("perturbed_one_iteration")["report"])
    rep = TC.reference("disparity")["report"]
    assert (rep[:, 0, 0] < full).all()     # the 0.01, the 0 and the NaN are no candidates
    # at the truth the step is small: the estimate stays within a fifth of a voxel and a fifth of a degree
    t, r = TC.pose_errors(TC.reference("truth")["c2w"], TC.cases()["truth"]["args"]["guess"])
    assert t.max() < 0.02 and r.max() < 0.0035


def test_init_and_poses_equal_the_oracle():
    """Shepperd's four branches, each with a rotation whose largest term is that branch's, and poses that are not quite
    rotations"""
    rng = np.random.default_rng(3)
    c2w = [TC.pose(0.3, -0.2, (1.0, 2.0, 3.0)), TC.pose(np.pi - 0.01, 0.0, (0, 0, 0)), TC.pose(0.0, np.pi - 0.02, (0, 1, 0)),
           TC.pose(np.pi - 0.3, np.pi - 0.2, (5, 0, 0)), TC.pose(0.1, 0.2, (0, 0, 0), skew=1e-3)]
    c2w += [np.concatenate([np.linalg.qr(rng.standard_normal((3, 3)))[0], rng.standard_normal((3, 1))], 1) for _ in range(8)]
    c2w = np.stack(c2w)
    state, est = HT.init(c2w, TC.K)
    want_state, want_est = TO.init(c2w, TC.K)
    assert TC.same_bits(state, want_state) and TC.same_bits(est, want_est)
    largest = {int(np.argmax(np.abs(s[:4]))) for s in want_state}
    assert largest == {0, 1, 2, 3}
    assert TC.same_bits(HT.poses(state), TO.poses(want_state))
    proper = [i for i in range(len(c2w)) if np.linalg.det(c2w[i, :, :3]) > 0.5 and i != 4]
    assert np.abs(TO.poses(want_state)[proper] - c2w[proper]).max() < 1e-14
    assert est[0, 12] == 12 and est[0, 14] == 9.5 and est[0, 15] == 5.5


def test_frames_in_one_call_equal_frames_one_by_one():
    case, ref = TC.cases()["perturbed_odd_size"]["args"], TC.reference("perturbed_odd_size")
    for v in range(3):
        one = {k: (a[v:v + 1] if isinstance(a, np.ndarray) and a.shape != (3, 3) else a) for k, a in case.items()}
        got = HT.align(**one)
        for key in TC.KEYS:
            assert TC.same_bits(got[key], ref[key][v:v + 1]), (v, key)


def test_convergence_on_the_oracle():
    """Ten iterations from the perturbed guesses (off by 0.095 .. 0.099 in translation, one voxel being 0.1, and 0.017 rad,
    one degree) on the sphere in the room's corner, the sum over the three frames.

    Measured on the oracle (printed below).  Frames of 37 x 61: the translation error falls 269-fold (to 2e-4 .. 5e-4) and
    the rotation angle 41-fold (to 2e-4 .. 6e-4 rad); the rms residual per iteration is 0.0555, 0.0088, 0.0025, then
    0.0024 for the rest.  Frames of 12 x 20 (a pixel is 1 / 12 rad): 33-fold (to 0.002 .. 0.004) and 7.9-fold (to
    0.001 .. 0.003 rad); rms 0.0568, 0.0074, then 0.0045.  What is left is the model's own error: the trilinear surface of
    a sphere of radius five voxels.  Asserted: at least half of each measured factor, and an rms that does not grow
    between consecutive iterations by more than 1 % of its first value."""
    for odd, gain_t, gain_r in ((True, 269.0, 41.0), (False, 33.0, 7.9)):
        c = TC.convergence(odd)
        print(f"odd={odd}: translation {c['gain_t']:.1f}-fold, rotation {c['gain_r']:.1f}-fold, rms {c['rms']}")
        assert c["gain_t"] >= gain_t / 2 and c["gain_r"] >= gain_r / 2
        assert (np.diff(c["rms"]) <= 0.01 * c["rms"][0]).all()
