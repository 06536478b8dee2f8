"""The depth-visualisation kernels (csrc_dvis/*.hip, compiled unchanged against the host simulator) against the numpy
oracle (tests/depth_vis_oracle.py): scaled predictions and ranges bit for bit, pictures byte for byte, both precisions,
ragged sets at aligned and shifted offsets, every planted value, and nothing written outside the outputs."""
import numpy as np
import pytest

import _depth_vis_cases as C
import _hostsim_dvis as S
import depth_vis_oracle as O
from scsfm_hip import depth_vis as DV

TABLE = DV.MAGMA


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


def check_maps(maps, shift=0):
    T = maps[0].dtype.type
    got = S.depth_range(maps, shift)
    want = np.array([O.depth_range(m) for m in maps], T)
    assert same_bits(got.astype(T), want) and same_bits(got, want.astype(np.float64))
    pics = S.colourise(maps, got, shift)
    for m, p, (vmin, vmax) in zip(maps, pics, want):
        assert np.array_equal(p, O.colourise(m, vmin, vmax, TABLE))
    return got, pics


@pytest.mark.parametrize("dtype", C.DTYPES, ids=("f32", "f64"))
@pytest.mark.parametrize("shape", C.SMALL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_range_and_picture_on_every_shape(shape, dtype):
    check_maps([C.base(shape, dtype, seed=shape[1])])


@pytest.mark.parametrize("dtype", C.DTYPES, ids=("f32", "f64"))
@pytest.mark.parametrize("shift", (0, 1))
def test_ragged_set(dtype, shift):
    maps = C.ragged(dtype)
    got, pics = check_maps(maps, shift)
    one, _ = check_maps(maps[2:3])
    assert same_bits(got[2:3], one)  # an image's result does not depend on its neighbours


@pytest.mark.parametrize("dtype", C.DTYPES, ids=("f32", "f64"))
@pytest.mark.parametrize("plant", list(C.PLANTS))
def test_planted_values(plant, dtype):
    maps = list(C.planted(plant, dtype))
    got, pics = check_maps(maps)
    if plant == "nan_in_one_image":
        assert np.isnan(got[1]).all() and not pics[1].any() and pics[0].any() and pics[2].any()
    if plant == "constant":
        assert got[1, 0] == got[1, 1] and (pics[1] == TABLE[0]).all()
    if plant == "top6_equal":
        assert (pics[1] == TABLE[255]).all(axis=-1).mean() > 0.06  # xa == 256 exactly on the plateau
    if plant == "inf":
        assert np.isnan(got[0, 1]) and np.isfinite(got[0, 0]) and not pics[0].any()
        assert np.isfinite(got[1:]).all() and (pics[1][2, 2] == TABLE[255]).all()


@pytest.mark.parametrize("dtype", C.DTYPES, ids=("f32", "f64"))
def test_foreign_range_gives_under_and_over_colours(dtype):
    gt = C.base((19, 25), dtype, seed=4)
    vmin, vmax = O.depth_range(gt)
    ranges = np.array([[vmin, vmax]] * 3, np.float64)
    maps = [gt * dtype(1000), gt * dtype(0.001), gt]
    pics = S.colourise(maps, ranges)
    for m, p in zip(maps, pics):
        assert np.array_equal(p, O.colourise(m, vmin, vmax, TABLE))
    assert (pics[0] == TABLE[0]).all() and (pics[1] == TABLE[255]).all()
    black = S.colourise(maps, np.array([[np.nan, vmax], [vmin, np.nan], [np.nan, np.nan]]))
    assert not any(p.any() for p in black)


@pytest.mark.parametrize("gdt", C.DTYPES, ids=("gt32", "gt64"))
@pytest.mark.parametrize("pdt", C.DTYPES, ids=("pred32", "pred64"))
@pytest.mark.parametrize("shift", (0, 3))
def test_scaled_prediction(gdt, pdt, shift):
    rdt = np.result_type(gdt, pdt)
    pred = C.base((5, 8, 11), pdt, seed=9) * pdt(0.05)
    pred[1, 2, 3] = -1e-6
    pred[3, 0, 0] = np.nan
    sizes = ((13, 17), (5, 40), (8, 11), (1, 1), (16, 3))
    ratios = np.array([17.25, 0.3, 1.0, 4.0, np.nan]).astype(rdt)
    out = S.scaled_depths(pred, ratios, sizes, rdt, shift)
    for i, (H, W) in enumerate(sizes):
        want = O.scaled_prediction(pred[i], ratios[i], H, W, rdt)
        assert want.dtype == rdt and same_bits(out.map(i), want), i


def test_scaled_prediction_then_picture_is_the_composite_panel():
    gts, pred = C.eval_set("kitti", np.float32, np.float64)
    ratios = np.array([30.5, 28.0, 1.0, 31.75])
    ev = O.evaluated(pred)
    assert ev == [0, 1, 3]
    sizes = [gts[i].shape for i in ev]
    scaled = S.scaled_depths(pred[ev], ratios[ev], sizes, np.float64)
    pics = S.colourise(scaled, S.depth_range(scaled))
    want = O.composites(gts, pred, ratios, "kitti", C.photos(sizes), TABLE)
    for p, c, (H, W) in zip(pics, want, sizes):
        assert np.array_equal(p, c[H:])
