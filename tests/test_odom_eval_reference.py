"""The odometry oracle (tests/odom_eval_oracle.py) against the reference's own KittiEvalOdom, run through
tests/_odom_eval_ref.py with plotting stubbed out, on the fixtures' trajectories (KITTI sequences 04 and 10) for all five
alignment modes: the segment tables agree exactly in first frames, lengths and speeds, and every float to rtol 1e-12 (both
are float64 numpy; the slack covers np.sum's pairwise order against the reference's Python loops, BLAS / LAPACK's inverse
and matmul against the oracle's written-out ones, and LAPACK's SVD against the oracle's Jacobi).  Also: the committed
fixture tests/golden/odom_eval.npz is what the reference computes today, and the oracle reproduces the reference's
text."""
import os
import sys

import numpy as np
import pytest

import _odom_eval_ref as REF
import odom_eval_oracle as O

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

pytestmark = pytest.mark.skipif(not REF.available(), reason="the reference checkout is not on this machine")


@pytest.fixture(scope="module")
def trajectories():
    import make_odom_eval_golden as G
    return G.trajectories()


@pytest.mark.parametrize("alignment", O.ALIGNMENTS, ids=str)
def test_oracle_reproduces_reference(trajectories, alignment):
    import make_odom_eval_golden as G
    gts, preds = trajectories
    rec = REF.run(gts, preds, G.SEQS, alignment)
    ora = O.evaluate(gts, preds, alignment)
    for s, (seq, o) in enumerate(zip(G.SEQS, ora)):
        seg = rec["seg"][s]
        assert seg.shape == o["seg"].shape
        np.testing.assert_array_equal(seg[:, [0, 3, 4]], o["seg"][:, [0, 3, 4]])
        np.testing.assert_allclose(o["seg"][:, 1:3], seg[:, 1:3], rtol=1e-12, atol=0)
        np.testing.assert_allclose(o["summary"][:5], rec["summary"][s], rtol=1e-12, atol=0)
        assert O.segment_lines(seg) == rec["errors"][s]  # (the text of the reference's own numbers)
    summaries = [o["summary"] for o in ora]
    text = sum((O.console_lines(seq, sm) for seq, sm in zip(G.SEQS, summaries)), []) + O.copy_block(summaries)
    ref_lines = rec["stdout"].splitlines()
    assert len(text) == len(ref_lines)
    for a, b in zip(text, ref_lines):  # the printed floats carry 17 digits: compare them as numbers
        ha, _, va = a.rpartition("  ")
        hb, _, vb = b.rpartition("  ")
        if ha and ha == hb:
            assert float(va) == pytest.approx(float(vb), rel=1e-12)
        else:
            assert a == b
    assert O.result_txt(G.SEQS, summaries) == rec["result_txt"]
    ref_summ = [list(r) + [1.0, len(sg)] for r, sg in zip(rec["summary"], rec["seg"])]
    assert O.console_lines(G.SEQS[0], ref_summ[0]) == ref_lines[:6]
    assert O.copy_block(ref_summ) == ref_lines[-5:]


def test_short_sequence_prints_as_the_reference(trajectories):
    """No segment at all (the first 60 frames of sequence 04, ~85 m): the reference prints the integer 0 and 0.0."""
    gts, preds = trajectories
    g, p = gts[0][:60], preds[0][:60]
    rec = REF.run([g], [p], (4,), None)
    o = O.evaluate_sequence(g, p, None)
    assert len(o["seg"]) == 0 and rec["seg"][0].shape == (0, 5)
    lines = O.console_lines(4, o["summary"])
    assert lines[:3] == rec["stdout"].splitlines()[:3] and lines[1].endswith(" 0") and lines[2].endswith(" 0.0")
    assert O.result_txt((4,), [o["summary"]]).splitlines()[:3] == rec["result_txt"].splitlines()[:3]


def test_golden_fixture_is_the_references(trajectories, golden_dir):
    import make_odom_eval_golden as G
    gts, preds = trajectories
    d = np.load(os.path.join(golden_dir, "odom_eval.npz"))
    for seq, g, p in zip(G.SEQS, gts, preds):
        np.testing.assert_array_equal(d[f"gt_{seq:02}"], g)
        np.testing.assert_array_equal(d[f"pred_{seq:02}"], p)
    for alignment, name in G.NAMES.items():
        rec = REF.run(gts, preds, G.SEQS, alignment)
        for seq, seg in zip(G.SEQS, rec["seg"]):
            np.testing.assert_array_equal(d[f"seg_{name}_{seq:02}"], seg)
        np.testing.assert_array_equal(d[f"summary_{name}"], rec["summary"])
        assert str(d[f"result_{name}"]) == rec["result_txt"] and str(d[f"stdout_{name}"]) == rec["stdout"]
