"""The snippet oracle (tests/pose_snippet_oracle.py) against the reference's own generator and compute_pose_error, run
through tests/_pose_snippet_ref.py, on the fixtures' inputs (tools/make_pose_snippet_golden.py): ATE and the compensated
ground truth to rtol 1e-12 (both are float64 numpy; the slack covers np.sum's and BLAS's order against the oracle's
left-to-right sums, and LAPACK's inverse and matmul against the written-out ones).  RE gets an absolute term on top:
max |RE_oracle - RE_reference| measured on the four fixtures on the CPU is 5.64e-17 (RE itself is 1.3e-3 .. 8e-3), and 8 x
that, 4.6e-16, is allowed for other BLAS builds (tests/_pose_snippet_check.py).  Also: the committed fixture
tests/golden/pose_snippets.npz is what the reference computes today."""
import os
import sys

import numpy as np
import pytest

import _pose_snippet_check as C
import _pose_snippet_ref as REF
import pose_snippet_oracle as P

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

pytestmark = pytest.mark.skipif(not REF.available(), reason="the reference checkout is not on this machine")


@pytest.fixture(scope="module")
def made():
    import make_pose_snippet_golden as G
    data = G.inputs()
    return G, data, G.reference_outputs(data)


def test_oracle_reproduces_reference(made):
    G, data, ref = made
    gts = [data["gt_a"], data["gt_b"]]
    worst = 0.0
    for mode, dt in G.VARIANTS:
        o = P.evaluate([P.mats(data[f"vec_{mode}_{dt}_{n}"], mode) for n in "ab"], gts, G.L)
        want = ref[f"errors_{mode}_{dt}"]
        worst = max(worst, float(np.max(np.abs(o["errors"][:, 1] - want[:, 1]))))
        C.check_errors(o["errors"], want)
        C.check_gt(o["gt"], ref["gt_comp"], gts, G.L)
        mean, std = REF.stats(o["errors"])
        assert P.report_lines(mean, std)[3:] == P.report_lines(ref[f"mean_{mode}_{dt}"], ref[f"std_{mode}_{dt}"])[3:]
        np.testing.assert_allclose(P.stats(o["errors"]), np.concatenate([mean, std]).astype(np.float64), rtol=1e-5)
    print("max |RE_oracle - RE_reference|", worst)
    assert worst <= C.RE_ATOL


def test_the_loop_and_the_stacked_oracle_are_one(made):
    G, data, _ = made
    m = P.mats(data["vec_quat_f64_b"], "quat")
    a, b = P.evaluate_sequence(m, data["gt_b"], G.L), P.evaluate_sequence_loop(m, data["gt_b"], G.L)
    for k in ("pred", "gt", "errors"):
        np.testing.assert_array_equal(a[k], b[k])


def test_golden_fixture_is_the_references(made, golden_dir):
    _, data, ref = made
    d = np.load(os.path.join(golden_dir, "pose_snippets.npz"))
    assert set(d.files) == set(data) | set(ref)
    for k, v in {**data, **ref}.items():
        assert d[k].dtype == v.dtype
        np.testing.assert_array_equal(d[k], v)
