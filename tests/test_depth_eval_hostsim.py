"""The evaluation kernels (csrc_eval/*.hip) compiled with g++ against the host simulator (tests/_hostsim_eval.py) and run
through the C ABI of include/scsfm_eval.h on host pointers, against the numpy oracle (tests/depth_eval_oracle.py).

Counts, skip flags, medians and ratios must be exact.  The metrics agree to 1e-12 relative (the oracle sums in float64
with numpy's pairwise order, the kernels in their fixed order), except the terms built on float32 logarithms: glibc's
logf / log10f (here; the device's on the GPU) and numpy's SIMD ones may differ by a few ulp.  If every log value is off
by at most e, then rmse_log = ||d|| / sqrt(n) moves by at most 2e (triangle inequality on the difference vector d, both
logs of a pair may be float32) and log10 = mean|d10| by at most 2e.  The bound used is e = 4 ulp of the largest log
magnitude on [1e-3, 1e3] m, plus the 1e-12 relative."""
import numpy as np
import pytest

import _depth_eval_data as D
import _hostsim_eval as H
import depth_eval_oracle as O

DT = {"f32": np.float32, "f64": np.float64}


def log_bound(gd, pd, base10):
    if gd == np.float64 and pd == np.float64:
        return 0.0
    big = np.float32(np.log10(1e3) if base10 else np.log(1e3))
    return 2 * 4 * float(np.spacing(big))


def check(out, gts, pred, dataset):
    ref = O.evaluate(gts, pred, dataset)
    np.testing.assert_array_equal(out["flag"], ref["flag"])
    ev = ref["flag"] == 1
    np.testing.assert_array_equal(out["count"][ev], ref["count"][ev])
    np.testing.assert_array_equal(out["stats"][:, 0], ref["ratio"].astype(np.float64))
    np.testing.assert_array_equal(out["stats"][:, 1], ref["med_gt"].astype(np.float64))
    np.testing.assert_array_equal(out["stats"][:, 2], ref["med_pred"].astype(np.float64))
    gd, pd = np.asarray(gts[0]).dtype.type, pred.dtype.type
    m, r = out["metrics"], ref["metrics"]
    assert (np.isnan(m) == np.isnan(r)).all()
    for c, name in enumerate(O.COLUMNS):
        atol = log_bound(gd, pd, name == "log10") if name in ("rmse_log", "log10") else 0.0
        k = ~np.isnan(r[:, c])
        np.testing.assert_allclose(m[k, c], r[k, c], rtol=1e-12, atol=atol, err_msg=name)
    return ref


@pytest.mark.parametrize("pd", ["f64", "f32"])
@pytest.mark.parametrize("gd", ["f32", "f64"])
def test_kitti_ragged_all_dtypes(pd, gd):
    """Ragged GT of odd sizes, predictions smaller in both axes, the crop, ties (GT quantised to 1/256 m), one skipped
    prediction (mean -1) and one image without a valid pixel (NaN)."""
    gts, pred = D.kitti_set(5, seed=5, sizes=((47, 156), (45, 151), (46, 153)), pred_hw=(17, 53), density=0.3,
                            pred_dtype=DT[pd], gt_dtype=DT[gd])
    pred[3] = -1.0
    gts[1][:] = 0.0
    out = H.evaluate(gts, pred, "kitti")
    check(out, gts, pred, "kitti")
    assert list(out["flag"]) == [1, 1, 1, 0, 1] and out["count"][1] == 0
    assert np.isnan(out["metrics"][1]).all() and np.isnan(out["stats"][1]).all()


@pytest.mark.parametrize("pd,gd", [("f64", "f32"), ("f32", "f32"), ("f32", "f64"), ("f64", "f64")])
def test_nyu_dense_pred_larger_equal_smaller(pd, gd):
    for gt_hw, pred_hw in (((33, 41), (52, 67)), ((30, 40), (30, 40)), ((31, 43), (16, 21))):
        gts, pred = D.nyu_set(3, seed=6, gt_hw=gt_hw, pred_hw=pred_hw, pred_dtype=DT[pd], gt_dtype=DT[gd])
        check(H.evaluate(list(gts), pred, "nyu"), list(gts), pred, "nyu")


def test_tiny_counts_and_ties():
    """1, 2, 3, 4, 6 and 8 valid pixels (odd and even medians), middle values equal, the two middle order statistics
    on both sides of a run of duplicates; quantised predictions tie too."""
    rng = np.random.default_rng(7)
    gts, preds = [], []
    for vals in ([5.0], [3.0, 7.0], [4.0, 4.0, 9.0], [2.0, 6.0, 6.0, 6.0], [1.0, 2.0, 2.0, 3.0, 3.0, 8.0], [5.0] * 8):
        g = np.zeros((19, 23), np.float32)
        g.flat[rng.choice(19 * 23, len(vals), replace=False)] = vals
        gts.append(g)
        preds.append(np.round(rng.uniform(0.5, 2.0, (11, 13)) * 4) / 4)
    for pd in (np.float64, np.float32):
        pred = np.stack(preds).astype(pd)
        out = H.evaluate(gts, pred, "nyu")
        check(out, gts, pred, "nyu")
        np.testing.assert_array_equal(out["count"], [1, 2, 3, 4, 6, 8])


def test_kitti_crop_edges():
    """Every pixel valid: the count is exactly the crop rectangle int32([.40810811 H, .99189189 H, .03594771 W,
    .96405229 W])."""
    for Hh, W in ((49, 167), (375, 1242), (37, 28)):
        g = np.full((Hh, W), 10.0, np.float32)
        c = O.kitti_crop(Hh, W)
        pred = np.full((1, 8, 24), 2.0)
        out = H.evaluate([g], pred, "kitti")
        check(out, [g], pred, "kitti")
        assert out["count"][0] == (c[1] - c[0]) * (c[3] - c[2])


def test_mask_bounds_compare_in_gt_precision():
    """GT values at float32(1e-3) and at max_depth are outside the mask of a float32 map (numpy compares in the GT's
    dtype); a float64 map keeps float32(1e-3), which is above 1e-3 in double."""
    g = np.full((20, 30), 5.0, np.float32)
    g[0, :10] = np.float32(1e-3)
    g[1, :7] = 10.0
    pred = np.ones((1, 10, 15))
    assert H.evaluate([g], pred, "nyu")["count"][0] == 600 - 10 - 7
    assert H.evaluate([g.astype(np.float64)], pred, "nyu")["count"][0] == 600 - 7
    assert O.evaluate([g], pred, "nyu")["count"][0] == 600 - 10 - 7
    assert O.evaluate([g.astype(np.float64)], pred, "nyu")["count"][0] == 600 - 7


def test_chunking_and_repeat_bit_identical():
    gts, pred = D.kitti_set(4, seed=8, sizes=((40, 131), (41, 129)), pred_hw=(12, 40), density=0.5)
    a = H.evaluate(gts, pred, "kitti")
    b = H.evaluate(gts, pred, "kitti")
    parts = [H.evaluate(gts[i:i + 1], pred[i:i + 1], "kitti") for i in range(4)]
    for k in ("metrics", "stats", "count", "flag"):
        assert a[k].tobytes() == b[k].tobytes()
        assert a[k].tobytes() == np.concatenate([p[k] for p in parts]).tobytes()


def test_unaligned_offsets_read_element_wise():
    """GT offsets that are not multiples of 4 take the element-wise loads and give the same bits."""
    gts, pred = D.kitti_set(3, seed=9, sizes=((21, 63), (23, 61)), pred_hw=(9, 30), density=0.5)
    _, _, gh, gw = H.pack(gts)
    flat = np.concatenate([g.ravel() for g in gts])
    off = np.concatenate([[0], np.cumsum([g.size for g in gts])[:-1]]).astype(np.int64)
    assert (off % 4 != 0).any()
    a = H.evaluate(gts, pred, "kitti")
    b = H.evaluate(gts, pred, "kitti", buf=(flat, off, gh, gw))
    for k in ("metrics", "stats", "count", "flag"):
        assert a[k].tobytes() == b[k].tobytes()
