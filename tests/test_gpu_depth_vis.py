"""scsfm_hip.depth_vis on the GPU against the numpy oracle (tests/depth_vis_oracle.py) and the recorded reference results
(tests/golden/depth_vis.npz): scaled predictions and ranges bit for bit, pictures byte for byte, on the shapes, ragged
sets and planted values of tests/_depth_vis_cases.py; independence of chunking and of a second run; a non-contiguous
input and a non-default stream."""
import types

import numpy as np
import pytest
import torch

import _depth_vis_cases as C
import depth_eval_oracle as E
import depth_vis_oracle as O
import make_depth_vis_golden as G
from scsfm_hip import depth_vis as DV

pytestmark = pytest.mark.gpu
TABLE = DV.MAGMA


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


def dev(maps):
    return [torch.from_numpy(np.ascontiguousarray(m)).cuda() for m in maps]


def check_maps(maps, staged=None):
    T = maps[0].dtype.type
    ranges, pics = DV.depth_pictures(dev(maps) if staged is None else staged)
    assert ranges.is_cuda and ranges.dtype == torch.float64 and tuple(ranges.shape) == (len(maps), 2)
    got = ranges.cpu().numpy()
    want = np.array([O.depth_range(m) for m in maps], T)
    assert same_bits(got.astype(T), want) and same_bits(got, want.astype(np.float64))
    for m, p, (vmin, vmax) in zip(maps, pics, want):
        assert p.is_cuda and p.dtype == torch.uint8
        assert np.array_equal(p.cpu().numpy(), O.colourise(m, vmin, vmax, TABLE))
    return got, [p.cpu().numpy() for p in pics]


@pytest.mark.parametrize("dtype", C.DTYPES, ids=("f32", "f64"))
@pytest.mark.parametrize("shape", C.SMALL_SHAPES + (C.LARGE_SHAPE,), ids=lambda s: "x".join(map(str, s)))
def test_range_and_picture_on_every_shape(shape, dtype):
    check_maps([C.base(shape, dtype, seed=shape[1])])


def test_size_at_which_the_precisions_pick_different_order_statistics():
    """n = 2 207 542, the smallest size at which float32 and float64 floor (n - 1) * 0.95 differently (found on the CPU:
    tests/test_dvis_library.py); the host-side index must follow the map's precision.  Against np.percentile itself."""
    n = 2207542
    assert DV.percentile_index(n, np.float32)[0] != DV.percentile_index(n, np.float64)[0]
    x32 = C.base((1, n), np.float32, seed=6)
    for x in (x32, x32.astype(np.float64)):
        got = DV.depth_range(dev([x])).cpu().numpy()[0]
        inv = 1 / (x + 1e-6)
        assert same_bits(got.astype(x.dtype), np.array([inv.min(), np.percentile(inv, 95)], x.dtype))


@pytest.mark.parametrize("dtype", C.DTYPES, ids=("f32", "f64"))
def test_ragged_set_chunking_and_a_second_run(dtype):
    maps = C.ragged(dtype)
    got, pics = check_maps(maps)
    again, pics2 = check_maps(maps)
    assert same_bits(got, again) and all(np.array_equal(a, b) for a, b in zip(pics, pics2))
    for i0, i1 in ((0, 2), (2, 3), (3, 6)):  # other neighbours, other offsets
        part, ppics = check_maps(maps[i0:i1])
        assert same_bits(part, got[i0:i1]) and all(np.array_equal(a, b) for a, b in zip(ppics, pics[i0:i1]))


@pytest.mark.parametrize("dtype", C.DTYPES, ids=("f32", "f64"))
def test_unaligned_offsets(dtype):
    """A hand-made Ragged whose offsets are no multiples of 4 elements."""
    maps = C.ragged(dtype)
    r = DV.Ragged([m.shape for m in maps], torch.from_numpy(maps[0]).dtype, "cuda")
    shifted = r.off + np.arange(1, len(maps) + 1) * 5 + 1
    assert (shifted % 4 != 0).any() and (np.diff(shifted) >= r.hw[:-1]).all()
    r.off = shifted
    r.total = int(r.off[-1] + r.hw[-1])
    r.buf = torch.full((r.total + 8,), float("nan"), dtype=r.buf.dtype, device="cuda")
    r.d_off = torch.from_numpy(r.off).cuda()
    for i, m in enumerate(maps):
        r.map(i).copy_(torch.from_numpy(m))
    check_maps(maps, r)


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
        assert np.isnan(got[0, 1]) and not pics[0].any() and (pics[1][2, 2] == TABLE[255]).all()


@pytest.mark.parametrize("gdt", C.DTYPES, ids=("gt32", "gt64"))
@pytest.mark.parametrize("rdt", C.DTYPES, ids=("pred32", "pred64"))
def test_pair_pictures_with_zeros_in_the_ground_truth_and_foreign_ranges(gdt, rdt):
    gts = list(C.planted("zeros", gdt, (3, 19, 25)))
    for scale in (1.0, 1000.0, 0.001):  # in, entirely above (under colour) and entirely below (over colour) the range
        preds = [C.base(g.shape, rdt, seed=20 + i) * rdt(scale) for i, g in enumerate(gts)]
        ranges, pp, gp = DV.depth_pair_pictures(dev(preds), dev(gts))
        for i in range(3):
            want = O.pair_pictures(preds[i], gts[i], TABLE)
            assert np.array_equal(pp[i].cpu().numpy(), want[0]) and np.array_equal(gp[i].cpu().numpy(), want[1])
        if scale == 1000.0:
            assert all((p.cpu().numpy() == TABLE[0]).all() for p in pp)
        if scale == 0.001:
            assert all((p.cpu().numpy() == TABLE[255]).all() for p in pp[:2])


@pytest.mark.parametrize("gdt", C.DTYPES, ids=("gt32", "gt64"))
@pytest.mark.parametrize("pdt", C.DTYPES, ids=("pred32", "pred64"))
def test_scaled_prediction(gdt, pdt):
    rdt = np.result_type(gdt, pdt)
    pred = C.base((6, 8, 11), pdt, seed=9) * pdt(0.05)
    pred[1, 2, 3] = -1e-6
    pred[3, 0, 0] = np.nan
    sizes = ((13, 17), (5, 40), (8, 11), (1, 1), (16, 3), (375, 1242))
    ratios = np.array([17.25, 0.3, 1.0, 4.0, np.nan, 31.5]).astype(rdt)
    out = DV.scaled_depths(torch.from_numpy(pred).cuda(), ratios, sizes, torch.from_numpy(ratios).dtype)
    for i, (H, W) in enumerate(sizes):
        assert same_bits(out.map(i).cpu().numpy(), O.scaled_prediction(pred[i], ratios[i], H, W, rdt)), i
    part = DV.scaled_depths(torch.from_numpy(pred).cuda()[4:], ratios[4:], sizes[4:], torch.from_numpy(ratios).dtype)
    assert torch.equal(part.map(1), out.map(5))


def test_golden_reference_results():
    d = np.load(G.GOLDEN)
    assert np.array_equal(d["magma"], DV.MAGMA)
    for tag in ("f32", "f64"):
        _, pics = DV.depth_pictures(torch.from_numpy(d[f"maps_{tag}"]).cuda())
        assert np.array_equal(torch.stack(pics).cpu().numpy(), d[f"pictures_{tag}"])
        _, pp, gp = DV.depth_pair_pictures(torch.from_numpy(d[f"pair_pred_{tag}"]).cuda(),
                                           torch.from_numpy(d[f"gt_{tag}"]).cuda())
        want = d[f"pair_pictures_{tag}"]
        assert np.array_equal(torch.stack(pp).cpu().numpy(), want[:, 0])
        assert np.array_equal(torch.stack(gp).cpu().numpy(), want[:, 1])
    gts, pred = [d[f"eval_gt_{i}"] for i in range(4)], d["eval_pred"]
    ev = O.evaluated(pred)
    ratios = E.evaluate(gts, pred, "kitti")["ratio"]
    out = DV.scaled_depths(torch.from_numpy(pred[ev]).cuda(), ratios[ev], [gts[i].shape for i in ev], torch.float64)
    for k in range(len(ev)):
        assert same_bits(out.map(k).cpu().numpy(), d[f"eval_scaled_{k}"]), k


@pytest.mark.parametrize("dataset", ("kitti", "nyu"))
@pytest.mark.parametrize("gdt,pdt", ((np.float32, np.float32), (np.float32, np.float64), (np.float64, np.float32)),
                         ids=("f32-f32", "f32-f64", "f64-f32"))
def test_composites_do_not_depend_on_chunking(dataset, gdt, pdt):
    gts, pred = C.eval_set(dataset, gdt, pdt)
    r = E.evaluate(gts, pred, dataset)
    res = types.SimpleNamespace(ratio=r["ratio"], evaluated=r["flag"] == 1)
    sizes = DV.picture_sizes(res, gts)
    photos = C.photos(sizes)
    want = O.composites(gts, pred, r["ratio"], dataset, photos, TABLE)
    staged = [torch.from_numpy(p).cuda() for p in photos]
    whole = DV.composites(res, pred, gts, dataset, staged)
    parts = DV.composites(res, pred, gts, dataset, staged[:1]) + DV.composites(res, pred, gts, dataset, staged[1:], 1)
    assert len(whole) == len(want) == 3
    for k in range(3):
        assert np.array_equal(whole[k].cpu().numpy(), want[k]), k
        assert torch.equal(whole[k], parts[k])
    with pytest.raises(ValueError):
        DV.composites(res, pred, gts, dataset, [staged[0][:-1]])


def test_non_contiguous_input_and_non_default_stream():
    wide = C.base((3, 37, 60), np.float32, seed=6)
    maps = [np.ascontiguousarray(m[:, 3:56]) for m in wide]
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        staged = torch.from_numpy(wide).cuda()[:, :, 3:56]
        assert not staged.is_contiguous()
        ranges, pics = DV.depth_pictures(staged)
        canvas = torch.zeros((37, 2 * 53 + 1, 3), dtype=torch.uint8, device="cuda")
        DV.colourise(staged[:1], ranges[:1], [canvas[:, 53:106]])
    stream.synchronize()
    for m, p in zip(maps, pics):
        assert np.array_equal(p.cpu().numpy(), O.depth_picture(m, TABLE))
    c = canvas.cpu().numpy()
    assert np.array_equal(c[:, 53:106], O.depth_picture(maps[0], TABLE)) and not c[:, :53].any() and not c[:, 106:].any()
