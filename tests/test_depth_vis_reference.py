"""The numpy oracle (tests/depth_vis_oracle.py) against the reference's own depth_visualizer, depth_pair_visualizer and
evaluate_depth return value run live (tests/_depth_vis_ref.py; skipped when the reference or matplotlib is absent) and
against what they gave when tests/golden/depth_vis.npz was recorded.  Byte for byte and bit for bit; the percentile alone
against np.percentile."""
import os

import numpy as np
import pytest

import _depth_vis_cases as C
import _depth_vis_ref as R
import depth_vis_oracle as O
import make_depth_vis_golden as G
from scsfm_hip import depth_vis as DV

needs_reference = pytest.mark.skipif(not R.available(), reason="the reference (or matplotlib) is not on this machine")
TABLE = DV.MAGMA


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


@pytest.fixture(scope="module")
def golden():
    return np.load(G.GOLDEN)


def test_magma_table_equals_matplotlib_at_every_entry(golden):
    assert np.array_equal(golden["magma"], DV.MAGMA)
    mpl = pytest.importorskip("matplotlib")
    assert np.array_equal((np.array(mpl.colormaps["magma"].colors, dtype=np.float64) * 255).astype(np.uint8), DV.MAGMA)


@pytest.mark.parametrize("dtype", C.DTYPES, ids=("f32", "f64"))
def test_percentile_equals_numpy_bit_for_bit(dtype):
    rng = np.random.default_rng(5)
    sizes = list(range(1, 70)) + [15, 20, 21, 41, 1961, 8320, 466650]
    with np.errstate(all="ignore"):
        for n in sizes:
            a = (1 / rng.uniform(0.5, 80.0, n)).astype(dtype)
            assert same_bits(O.percentile95(a), np.percentile(a, 95)), n
            assert O.percentile_index(n, dtype) == DV.percentile_index(n, dtype)
        for a in (np.array([1, 2, np.inf, np.inf], dtype), np.array([np.inf] * 3, dtype), np.array([np.inf], dtype),
                  np.array([3, np.nan, 1], dtype), np.array([-np.inf, 0, 5, 5, 5], dtype)):
            assert same_bits(O.percentile95(a), np.percentile(a, 95)), a


def test_percentile_where_the_precisions_pick_different_elements():
    """n = 2 207 542 is the smallest size at which float32 and float64 floor the virtual index (n - 1) * 0.95 to
    different order statistics (float32 has a spacing of 0.25 there and rounds 2097413.95 up to 2097414.0); below it
    only the weight differs.  Both precisions against numpy."""
    n = 2207542
    a32 = (1 / np.random.default_rng(6).uniform(0.5, 80.0, n)).astype(np.float32)
    assert same_bits(O.percentile95(a32), np.percentile(a32, 95))
    a64 = a32.astype(np.float64)
    assert same_bits(O.percentile95(a64), np.percentile(a64, 95))
    assert O.percentile_index(n, np.float32)[0] != O.percentile_index(n, np.float64)[0]


def test_oracle_equals_the_golden(golden):
    for name, want in G.oracle_outputs(golden).items():
        assert same_bits(want, golden[name]), name
    assert os.path.getsize(G.GOLDEN) < 100 * 1024


@needs_reference
def test_golden_is_what_the_reference_gives_now(golden):
    for name, want in G.reference_outputs(golden).items():
        assert same_bits(want, golden[name]), name


@needs_reference
@pytest.mark.parametrize("dtype", C.DTYPES, ids=("f32", "f64"))
@pytest.mark.parametrize("shape", C.SMALL_SHAPES + (C.SPLIT_SHAPE, C.LARGE_SHAPE), ids=lambda s: "x".join(map(str, s)))
def test_picture_equals_the_live_reference(shape, dtype):
    x = C.base(shape, dtype, seed=shape[1])
    assert np.array_equal(O.depth_picture(x, TABLE), R.depth_visualizer(x))


@needs_reference
@pytest.mark.parametrize("dtype", C.DTYPES, ids=("f32", "f64"))
@pytest.mark.parametrize("plant", list(C.PLANTS))
def test_planted_values_equal_the_live_reference(plant, dtype):
    for i, x in enumerate(C.planted(plant, dtype)):
        assert np.array_equal(O.depth_picture(x, TABLE), R.depth_visualizer(x)), i


@needs_reference
@pytest.mark.parametrize("gdt", C.DTYPES, ids=("gt32", "gt64"))
@pytest.mark.parametrize("rdt", C.DTYPES, ids=("pred32", "pred64"))
def test_pair_pictures_equal_the_live_reference(gdt, rdt):
    gts = C.planted("zeros", gdt, (3, 19, 25))
    for i, gt in enumerate(gts):
        for scale in (1.0, 1000.0, 0.001):  # in, entirely above and entirely below the ground truth's range
            pred = C.base(gt.shape, rdt, seed=20 + i) * rdt(scale)
            got = O.pair_pictures(pred, gt, TABLE)
            want = R.depth_pair_visualizer(pred, gt)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (i, scale)


@needs_reference
@pytest.mark.parametrize("dataset", ("kitti", "nyu"))
@pytest.mark.parametrize("gdt", C.DTYPES, ids=("gt32", "gt64"))
@pytest.mark.parametrize("pdt", C.DTYPES, ids=("pred32", "pred64"))
def test_scaled_prediction_equals_what_evaluate_depth_returns(dataset, gdt, pdt):
    import depth_eval_oracle as E
    gts, pred = C.eval_set(dataset, gdt, pdt)
    want = R.resized_predictions(gts, pred, dataset)
    ev = O.evaluated(pred)
    assert ev == [0, 1, 3] and len(want) == 3
    ratios = E.evaluate(gts, pred, dataset)["ratio"]
    rdt = np.result_type(gdt, pdt)
    for k, i in enumerate(ev):
        H, W = gts[i].shape
        assert same_bits(O.scaled_prediction(pred[i], ratios[i], H, W, rdt), want[k]), i
