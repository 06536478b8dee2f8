"""The validation-log kernels (csrc_vlog/), compiled unchanged for the host simulator, against what the reference
recorded in tests/golden/validation_log.npz: the float pictures bit for bit (NaN for NaN), the byte pictures equal to the
float pictures pushed through the byte rule, on outputs that start as 0xAB so that an unwritten byte shows, with the
buffers on and off the 16-byte boundary."""
import numpy as np
import pytest

import _hostsim_vlog as H
import _validation_log_golden as G
import validation_log_oracle as O

OFFSETS = (0, 4, 8)


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


def as_pixels(floats):
    """float [N, C, H, W] -> the bytes [N, H, W, C] the library writes beside it."""
    return np.ascontiguousarray(O.to_bytes(floats).transpose(0, 2, 3, 1))


@pytest.mark.parametrize("offset", OFFSETS)
@pytest.mark.parametrize("key", ["a", "b", "c"])
def test_map_pictures_equal_the_golden(key, offset):
    g = G.load()
    maps = g[f"maps_{key}"]
    for cmap, max_value in G.CALLS:
        want = g[f"{key}/{cmap}"]
        floats, rgba = H.map_pictures(maps, g[cmap], max_value, offset=offset)
        assert same(floats, want), (cmap, np.argwhere(floats != want)[:4].tolist())
        assert same(rgba, as_pixels(want)), cmap
        # either output alone
        assert same(H.map_pictures(maps, g[cmap], max_value, bytes_=False, offset=offset)[0], want)
        assert same(H.map_pictures(maps, g[cmap], max_value, floats=False, offset=offset)[1], rgba)


def test_what_the_maps_hold():
    """The golden pictures show what their maps were chosen for."""
    g = G.load()
    a, magma, rainbow = g["maps_a"], g["magma"], g["rainbow"]
    pics = g["a/magma"]
    assert np.argmax(a[1]) == a[1].size - 1 and (pics[1, :, -1, -1] == magma[-1]).all()
    assert (pics[1, :, 2, 3] == magma[0]).all()                         # a negative value: the under colour
    assert (pics[2, :, 5, 7] == magma[0]).all() and (pics[2, :, 0, 0] == magma[0]).all()  # +0 and -0
    assert np.isnan(a[3]).sum() == 1 and not pics[3].any()              # a NaN maximum blanks the image
    assert not a[4].any() and not pics[4].any()                         # 0 / 0
    assert np.isinf(a[5]).sum() == 1 and not pics[5, :, 3, 3].any()     # inf / inf; every other pixel is x / inf = 0
    assert (pics[5].reshape(4, -1).T == magma[0]).all(axis=1).sum() == a[5].size - 1
    assert len({tuple(p[:, 0, 0]) for p in pics[:2]}) == 2
    b, pics = g["maps_b"], g["b/rainbow"]
    assert b[1, 1, 2] == 10 and (pics[1, :, 1, 2] == rainbow[-1]).all()  # xa == table_n
    assert (pics[1, :, 2, 3] == rainbow[-1]).all() and (pics[1, :, 7, 15] == rainbow[-1]).all()
    assert (pics[1, :, 0, 0] == rainbow[0]).all() and (pics[1, :, 4, 4] == rainbow[-1]).all()
    assert (g["gt/depth_picture"][:, 3] <= 1).all() and g["c/magma"].shape == (1, 4, 1, 1)


@pytest.mark.parametrize("offset", OFFSETS)
def test_maxima(offset):
    g = G.load()
    for key in "abc":
        maps = g[f"maps_{key}"]
        with np.errstate(invalid="ignore"):
            want = maps.reshape(len(maps), -1).max(axis=1)
        got = H.image_max(maps, offset)
        assert got.shape == want.shape and bool(np.all((got == want) | (np.isnan(got) & np.isnan(want)))), key
    neg = -np.abs(g["maps_b"]) - np.float32(1e-3)  # all negative, more pixels than one block folds in one step
    big = np.tile(neg, (1, 20, 20))
    big[1, 159, 319] = -1e-30
    assert same(H.image_max(big, offset), big.reshape(2, -1).max(axis=1))


@pytest.mark.parametrize("offset", OFFSETS)
def test_input_picture_on_every_byte_value(offset):
    g = G.load()
    batch, want = g["batch"], g["batch/floats"]
    floats, rgb = H.input_pictures(batch, offset=offset)
    assert same(floats, want)
    assert same(rgb, as_pixels(want))
    assert same(H.input_pictures(batch, bytes_=False, offset=offset)[0], want)
    assert same(H.input_pictures(batch, floats=False, offset=offset)[1], rgb)
    # the 256 byte values come back as themselves or one below (0.45 + x * 0.225 is not the inverse, bit for bit), the
    # planted values clamp, and a fused multiply-add would have given other bits
    k = (np.arange(330) % 256).reshape(2, 3, 5, 11).transpose(0, 2, 3, 1)
    planted = np.zeros(k.shape, bool)
    planted[1, 4, 8:, 2] = True
    assert ((k - rgb.astype(int))[~planted] >= 0).all() and ((k - rgb.astype(int))[~planted] <= 1).all()
    assert rgb[1, 4, 8:, 2].tolist() == [0, 255, 0]
    fused = (np.float64(np.float32(0.45)) + batch.astype(np.float64) * np.float64(np.float32(0.225))).astype(np.float32)
    assert (fused != want)[~np.isnan(want)].sum() >= 30


@pytest.mark.parametrize("offset", OFFSETS)
def test_target_disparity_and_its_pictures(offset):
    g = G.load()
    gt = g["gt"]
    disp = H.target_disparity(gt, offset)
    assert same(disp, g["gt/disparity"])
    assert disp[0, 0, 0] == np.float32(1 / np.float32(1000)) and disp[0, 0, 1] == 10 and disp[0, 2, 2] == 0
    assert np.isnan(disp[1, 3, 3]) and disp[1, 4, 4] == 0 and disp[1, 5, 5] == 10
    assert same(H.map_pictures(gt, g["rainbow"], 10, offset=offset)[0], g["gt/depth_picture"])
    assert same(H.map_pictures(disp, g["magma"], None, offset=offset)[0], g["gt/disparity_picture"])
    assert g["gt/disparity_picture"][0].any() and not g["gt/disparity_picture"][1].any()


def test_oracle_equals_the_golden():
    """The numpy restatement the GPU tests use for train.py's files."""
    g = G.load()
    for key in "abc":
        for cmap, max_value in G.CALLS:
            assert same(O.map_pictures(g[f"maps_{key}"], g[cmap], max_value), g[f"{key}/{cmap}"])
    assert same(O.input_pictures(g["batch"]), g["batch/floats"])
    assert same(O.target_disparity(g["gt"]), g["gt/disparity"])
