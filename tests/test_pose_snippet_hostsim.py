"""The snippet kernels (csrc_snip/*.hip) compiled with g++ against the host simulator (tests/_hostsim_snip.py) and run
through the C ABI of include/scsfm_snip.h on host pointers, against the numpy oracle (tests/pose_snippet_oracle.py) and
the reference's recorded results (tests/golden/pose_snippets.npz).  The tolerances and their basis are in
tests/_pose_snippet_check.py.  The oracle is fed the pair matrices the simulator's own pose_vec2mat forms (csrc_odom's
`local` output: the same closed forms under the same compiler), so that numpy's sin / cos are not part of the comparison."""
import os

import numpy as np
import pytest

import _hostsim_odom as HO
import _hostsim_snip as H
import _pose_snippet_check as C
import pose_snippet_oracle as P

VARIANTS = [(mode, dt) for mode in ("euler", "quat") for dt in ("f32", "f64")]


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "pose_snippets.npz"))


def _fixture(d, mode, dt):
    return [d[f"vec_{mode}_{dt}_{n}"] for n in "ab"], [d["gt_a"], d["gt_b"]]


def _mats(vecs, mode):
    return [m.astype(np.float64) for m in HO.chain(vecs, mode)[1]]


@pytest.mark.parametrize("mode,dt", VARIANTS, ids=[f"{m}-{d}" for m, d in VARIANTS])
def test_fixture_against_oracle_and_reference(golden, mode, dt):
    vecs, gts = _fixture(golden, mode, dt)
    out = H.evaluate(vecs, gts, 5, mode)
    want = P.evaluate(_mats(vecs, mode), gts, 5)
    assert out["errors"].shape == (65 + 69, 2) and np.isfinite(out["errors"]).all()
    report = []
    C.check_errors(out["errors"], want["errors"], report)
    C.check_pred(out["pred"], want["pred"])
    C.check_gt(out["gt"], want["gt"], gts, 5)
    # the double statistics against the oracle's, and against the reference's float32 mean and std: numpy's float32
    # sum over <= 2,000 values errs by about (log2 n + 1) 6e-8 < 1e-6, and the fixture keeps std >= mean / 5, so the std
    # is not the small difference of large numbers
    ref = np.concatenate([golden[f"mean_{mode}_{dt}"], golden[f"std_{mode}_{dt}"]]).astype(np.float64)
    print(report, "stats", out["stats"], "reference", ref)
    np.testing.assert_allclose(out["stats"], P.stats(want["errors"]), rtol=1e-12, atol=0)
    np.testing.assert_allclose(out["stats"], ref, rtol=1e-5, atol=0)
    # the reference's own numbers: the compensated ground truth, and (float64 vectors: no float32 sin / cos between the
    # two) the errors per snippet
    C.check_gt(out["gt"], golden["gt_comp"], gts, 5)
    if dt == "f64":
        C.check_errors(out["errors"], golden[f"errors_{mode}_{dt}"])


def test_ragged_set_across_wave_and_workgroup_boundaries():
    vecs, gts = C.ragged_set()
    out = H.evaluate(vecs, gts, 5, "euler")
    want = P.evaluate(_mats(vecs, "euler"), gts, 5)
    assert len(out["errors"]) == 0 + 0 + 1 + 2 + 64 + 65 + 256 + 257
    assert np.isfinite(out["errors"]).all() and np.isfinite(out["pred"]).all() and np.isfinite(out["gt"]).all()
    C.check_errors(out["errors"], want["errors"])
    C.check_pred(out["pred"], want["pred"])
    C.check_gt(out["gt"], want["gt"], gts, 5)
    np.testing.assert_allclose(out["stats"], P.stats(want["errors"]), rtol=1e-12, atol=0)


@pytest.mark.parametrize("seq_len", [3, 7])
def test_other_snippet_lengths(golden, seq_len):
    vecs, gts = [golden["vec_euler_f32_a"]], [golden["gt_a"]]
    out = H.evaluate(vecs, gts, seq_len, "euler")
    want = P.evaluate(_mats(vecs, "euler"), gts, seq_len)
    assert out["pred"].shape == (69 - seq_len + 1, seq_len, 3, 4)
    C.check_errors(out["errors"], want["errors"])
    C.check_pred(out["pred"], want["pred"])
    C.check_gt(out["gt"], want["gt"], gts, seq_len)
    np.testing.assert_allclose(out["stats"], P.stats(want["errors"]), rtol=1e-12, atol=0)


def test_repeat_grouping_and_null_gt_comp_give_the_same_bytes(golden):
    vecs, gts = C.ragged_set(np.float32)
    fv, fg = _fixture(golden, "euler", "f32")
    vecs, gts = [fv[0]] + vecs + [fv[1]], [fg[0]] + gts + [fg[1]]
    a = H.evaluate(vecs, gts, 5, "euler")
    b = H.evaluate(vecs, gts, 5, "euler")
    c = H.evaluate(vecs, gts, 5, "euler", with_gt_comp=False)
    assert c["gt"] is None
    for k in ("errors", "pred", "stats"):
        assert a[k].tobytes() == b[k].tobytes() == c[k].tobytes()
    assert a["gt"].tobytes() == b["gt"].tobytes()
    at = 0
    for v, g in zip(vecs, gts):
        n = max(len(g) - 4, 0)
        if n:
            one = H.evaluate([v], [g], 5, "euler")
            for k in ("errors", "pred", "gt"):
                assert one[k].tobytes() == a[k][at:at + n].tobytes()
        at += n
    assert at == len(a["errors"])
