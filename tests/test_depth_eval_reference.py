"""The depth-evaluation oracle (tests/depth_eval_oracle.py) against the reference's own code: eval_depth.py's
compute_depth_errors and DepthEvalEigen.evaluate_depth, pulled out with ast and run on real numpy with the oracle's
INTER_LINEAR as cv2.resize (tests/_depth_eval_ref.py).  The masked / scaled / clamped pairs that reach
compute_depth_errors must be the oracle's bit for bit, the ratios too; the errors agree to the summation: the reference
means in the promoted dtype (numpy's pairwise sum), the oracle in float64, so float64 inputs agree to 1e-12 and float32
ones to float32's pairwise-sum error (1e-5 relative here).  The printed table and ratio lines are compared as text.
Also: the committed fixtures tests/golden/depth_eval_*.npz are what the reference computes today."""
import os
import sys

import numpy as np
import pytest

import _depth_eval_data as D
import _depth_eval_ref as REF
import depth_eval_oracle as O

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

pytestmark = pytest.mark.skipif(not REF.available(), reason="the reference checkout is not on this machine")

SMALL_KITTI = ((47, 156), (46, 153), (47, 155), (48, 157))


def _cases():
    for pd in (np.float64, np.float32):
        for gd in (np.float32, np.float64):
            yield "kitti", pd, gd
            yield "nyu", pd, gd


def _set(dataset, pd, gd, seed):
    if dataset == "kitti":
        gts, pred = D.kitti_set(6, seed=seed, sizes=SMALL_KITTI, pred_hw=(16, 52), density=0.25, pred_dtype=pd,
                                gt_dtype=gd)
        pred[1] = -1.0  # skipped by the reference
        return gts, pred
    return D.nyu_set(5, seed=seed, gt_hw=(48, 64), pred_hw=(26, 32), pred_dtype=pd, gt_dtype=gd)


@pytest.mark.parametrize("dataset,pd,gd", list(_cases()), ids=lambda v: getattr(v, "__name__", v))
def test_oracle_reproduces_reference(dataset, pd, gd):
    gts, pred = _set(dataset, pd, gd, seed=3)
    rec = REF.run(gts, pred, dataset)
    ora = O.evaluate(gts, pred, dataset)
    ev = np.flatnonzero(ora["flag"] == 1)
    assert len(rec["pairs"]) == len(ev)
    for (rg, rp), i in zip(rec["pairs"], ev):  # what reaches compute_depth_errors: identical
        vg, vp = O.valid_pairs(gts[i], pred[i], dataset)
        ratio = np.median(vg) / np.median(vp)
        vp = (vp * ratio).astype(vp.dtype)
        vp = np.clip(vp, np.asarray(1e-3, vp.dtype), np.asarray(O.MAX_DEPTH[dataset], vp.dtype))
        assert rg.dtype == vg.dtype and rp.dtype == vp.dtype
        np.testing.assert_array_equal(rg, vg)
        np.testing.assert_array_equal(rp, vp)
    assert rec["ratios"].dtype == ora["ratios"].dtype
    np.testing.assert_array_equal(rec["ratios"], ora["ratios"])
    cols = [O.COLUMNS.index(c) for c in O.DATASET_COLUMNS[dataset]]
    rtol = 1e-12 if np.result_type(pd, gd) == np.float64 else 1e-5
    np.testing.assert_allclose(np.array(rec["errors"], np.float64), ora["metrics"][ev][:, cols], rtol=rtol, atol=0)
    lines = rec["stdout"].splitlines()
    assert lines[0] == "==> Evaluating depth result..."
    ours = O.report_lines(dataset, ora["mean"], ora["ratio_stats"])
    assert lines[1:3] == ours[:2]  # ratio statistics: the same numpy calls on the same ratios
    assert lines[3:] == ours[2:] or rtol > 1e-12  # (the table's 3 decimals hold unless a mean sits on a rounding edge)


def test_reference_empty_mask_gives_nan():
    gts, pred = _set("kitti", np.float64, np.float32, seed=4)
    gts[2][:] = 0.0
    rec = REF.run(gts, pred, "kitti")
    ora = O.evaluate(gts, pred, "kitti")
    assert np.isnan(ora["ratio"][2]) and np.isnan(ora["metrics"][2]).all() and ora["flag"][2] == 1
    assert np.isnan(rec["ratios"]).sum() == 1 and np.isnan(np.array(rec["errors"])[1]).all()  # (image 1 is skipped)


def test_resize_matches_opencv_rules():
    """Spot checks of the written-out INTER_LINEAR: identity at equal size, edge replication, an exact midpoint."""
    rng = np.random.default_rng(0)
    a = rng.random((7, 9))
    np.testing.assert_array_equal(O.resize_linear(a, 9, 7), a)
    up = O.resize_linear(np.array([[1.0, 3.0]]), 4, 1)  # x: -0.25 -> edge, 0.25, 0.75, 1.25 -> edge
    np.testing.assert_array_equal(up, [[1.0, 1.5, 2.5, 3.0]])
    down = O.resize_linear(np.array([[0.0, 2.0, 4.0, 6.0]], np.float32), 2, 1)  # x: 0.5, 2.5
    np.testing.assert_array_equal(down, np.array([[1.0, 5.0]], np.float32))


@pytest.mark.parametrize("name", ["kitti", "nyu"])
def test_golden_fixtures_are_the_references(name, golden_dir):
    import make_depth_eval_golden as G
    gts, pred = G.sets()[name]
    d = np.load(os.path.join(golden_dir, f"depth_eval_{name}.npz"))
    flat = np.concatenate([np.asarray(g).ravel() for g in gts])
    np.testing.assert_array_equal(d["gt"], flat)
    np.testing.assert_array_equal(d["pred"], pred)
    rec = REF.run(gts, pred, name)
    np.testing.assert_array_equal(d["errors"], np.array(rec["errors"]))
    np.testing.assert_array_equal(d["ratios"], rec["ratios"])
    assert str(d["stdout"]) == rec["stdout"]
