"""The odometry kernels (csrc_odom/*.hip) compiled with g++ against the host simulator (tests/_hostsim_odom.py) and run
through the C ABI of include/scsfm_odom.h on host pointers, against the numpy oracle (tests/odom_eval_oracle.py) and the
reference's recorded results (tests/golden/odom_eval.npz).  The judgement and the derivation of every tolerance are in
tests/_odom_eval_check.py: segment counts, first frames, lengths, speeds and per-length counts exact; floats to the
summation-order and arccos bounds evaluated on the data."""
import os

import numpy as np
import pytest

import _hostsim_odom as H
import _odom_eval_check as C
import odom_eval_oracle as O

NAMES = {None: "none", "scale": "scale", "scale_7dof": "scale_7dof", "7dof": "7dof", "6dof": "6dof"}


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "odom_eval.npz"))


def _fixture_sets(d):
    return [d["gt_04"], d["gt_10"]], [d["pred_04"], d["pred_10"]]


def synthetic(seed=3):
    """A ragged set: one frame, two frames, 60 frames of 1.2 m (72 m: no segment), a 400-frame curve, and its mirror
    image as the prediction of a fifth sequence (Umeyama's reflection fix)."""
    rng = np.random.default_rng(seed)

    def traj(n, step, noise=0.0, mirror=False):
        vec = np.zeros((max(n - 1, 0), 6))
        vec[:, 2] = -step
        vec[:, 4] = 0.004 + 0.002 * np.sin(np.arange(max(n - 1, 0)) / 17.0)
        vec[:, 3] = 0.001 * np.cos(np.arange(max(n - 1, 0)) / 11.0)
        g = O.fold(O.euler_mat(vec))
        p = O.fold(O.euler_mat(vec * 0.05 + np.concatenate([np.zeros((len(vec), 3)), vec[:, 3:] * 0.95], 1)
                               + rng.normal(0, noise, vec.shape)))
        if mirror:
            p[:, 0, 3] = -p[:, 0, 3]
        return g.reshape(-1, 12), p.reshape(-1, 12)

    sets = [traj(1, 1.2), traj(2, 1.2, 1e-4), traj(60, 1.2, 1e-4), traj(400, 1.1, 2e-4), traj(400, 1.1, 2e-4, True)]
    return [g for g, _ in sets], [p for _, p in sets]


@pytest.mark.parametrize("alignment", O.ALIGNMENTS, ids=str)
def test_fixtures_against_oracle_and_golden(golden, alignment):
    gts, preds = _fixture_sets(golden)
    out = H.evaluate(gts, preds, alignment)
    C.check_set(out, gts, preds, alignment)
    assert list(out["n_seg"]) == [43, 464]
    assert out["per_length"][0][4:, 2].sum() == 0  # sequence 04 is 394 m long: no segment of 500 m or more
    name = NAMES[alignment]
    for s, seq in enumerate((4, 10)):
        want = golden[f"seg_{name}_{seq:02}"]
        np.testing.assert_array_equal(out["seg"][s][:len(want), [0, 3, 4]], want[:, [0, 3, 4]])


def test_general_inverse_not_a_transpose(golden):
    """KITTI's GT rotations are orthonormal only to 1e-7: with a rigid-transpose inverse the translation error of
    sequence 10 without alignment is off by ~1e-7 relative; it must match the reference's recorded value to 1e-10."""
    gts, preds = _fixture_sets(golden)
    out = H.evaluate(gts[1:], preds[1:], None)
    want = golden["summary_none"][1]
    np.testing.assert_allclose(out["summary"][0][0], want[0], rtol=1e-10, atol=0)
    np.testing.assert_allclose(out["seg"][0][:464, 2], golden["seg_none_10"][:, 2], rtol=1e-10, atol=0)


@pytest.mark.parametrize("alignment", O.ALIGNMENTS, ids=str)
def test_synthetic_ragged_sets(alignment):
    gts, preds = synthetic()
    out = H.evaluate(gts, preds, alignment)
    refs = C.check_set(out, gts, preds, alignment)
    assert list(out["n_seg"][:3]) == [0, 0, 0] and out["n_seg"][3] > 0
    assert np.isnan(out["summary"][0][3:5]).all()  # RPE of a single frame: the mean of nothing
    assert (out["summary"][:3, :2] == 0).all()
    if alignment in ("7dof", "6dof", "scale_7dof"):
        assert refs[4]["info"]["s3"] == -1.0 and refs[3]["info"]["s3"] == 1.0


def test_together_and_one_by_one_are_byte_identical(golden):
    gts, preds = _fixture_sets(golden)
    sg, sp = synthetic()
    gts, preds = [gts[0]] + sg + [gts[1]], [preds[0]] + sp + [preds[1]]
    for alignment in (None, "7dof", "scale"):
        a = H.evaluate(gts, preds, alignment)
        b = H.evaluate(gts, preds, alignment)
        for s in range(len(gts)):
            one = H.evaluate(gts[s:s + 1], preds[s:s + 1], alignment)
            n = one["n_seg"][0]
            assert a["n_seg"][s] == n == b["n_seg"][s]
            for k in ("summary", "per_length"):
                assert a[k][s].tobytes() == one[k][0].tobytes() == b[k][s].tobytes()
            assert a["seg"][s][:n].tobytes() == one["seg"][0][:n].tobytes() and not a["seg"][s][n:].any()
            for k in ("gt_rel", "aligned"):
                assert a[k][s].tobytes() == one[k][0].tobytes() == b[k][s].tobytes()


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("mode", ["euler", "quat"])
def test_chain_against_the_sequential_fold(dtype, mode):
    """Ragged: no vector at all, one, a wave, across waves, across workgroups (1,590 vectors: sequence 09's length).  The
    local matrices against numpy's pose_vec2mat: sin / cos / sqrt of the two libraries within 2 ulp each and four
    roundings per entry, entries <= 1 -> 8 ulp of 1 in the input precision.  The chain against the fold of those very
    matrices: n eps max|position|."""
    rng = np.random.default_rng(5)
    vecs = []
    for n in (0, 1, 64, 200, 257, 1590):
        v = rng.normal(0, 0.01, (n, 6))
        v[:, 2] -= 0.4
        vecs.append(v.astype(dtype))
    poses, local = H.chain(vecs, mode)
    report = []
    for v, g, l in zip(vecs, poses, local):
        assert g.shape == (len(v) + 1, 3, 4) and l.dtype == dtype
        want = (O.euler_mat if mode == "euler" else O.quat_mat)(v)
        assert len(v) == 0 or np.abs(l - want).max() <= 8 * np.finfo(dtype).eps
        np.testing.assert_array_equal(l[:, :, 3], v[:, :3])
        C.check_chain(g, l, report)
    assert report[-1][1] <= 2e-10  # (the issue's figure for 1,591 frames)
    again, _ = H.chain(vecs[::-1], mode)
    for a, b in zip(poses, again[::-1]):
        assert a.tobytes() == b.tobytes()
