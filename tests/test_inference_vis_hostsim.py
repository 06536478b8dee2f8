"""The visualisation kernels (csrc_vis/), compiled unchanged for the host simulator, against the numpy oracle: byte for
byte and bit for bit, on outputs that start as 0xAB so that an unwritten byte shows."""
import numpy as np
import pytest
import torch

import _hostsim_vis as H
import _inference_vis_cases as C
import inference_vis_oracle as O


def same_floats(a, b):
    """Equal bits, except that NaNs match NaNs and -0 matches +0 (the maximum may return either zero)."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


def check_pictures(maps, colourise):
    for name, max_value, reciprocal in C.CALLS:
        got = colourise(maps, name, max_value, reciprocal)
        want = O.colourise(maps, name, max_value, reciprocal)
        assert got.shape == want.shape == maps.shape + (4,) and got.dtype == np.uint8
        bad = np.argwhere((got != want).any(axis=-1))
        assert len(bad) == 0, (name, max_value, reciprocal, len(bad), bad[:4].tolist())


@pytest.mark.parametrize("shape", C.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_pictures_on_every_shape(shape):
    maps = C.base(shape)
    assert same_floats(H.image_max(maps), O.image_max(maps))
    check_pictures(maps, H.colourise)
    if shape[0] == 3:
        assert len(set(O.image_max(maps).tolist())) == 3  # three images, three maxima
        assert not np.array_equal(O.colourise(maps, "bone"), O.colourise(maps / maps.max(), "bone", max_value=1))


@pytest.mark.parametrize("plant", list(C.PLANTS))
def test_planted_values(plant):
    maps = C.planted(plant)
    assert same_floats(H.image_max(maps), O.image_max(maps))
    check_pictures(maps, H.colourise)


def test_what_the_planted_cases_hold():
    """The cases exercise what they are named after (judged on the oracle, which the reference test ties to
    matplotlib)."""
    bone, rainbow = O.table("bone"), O.table("rainbow")
    m = C.planted("max_last")
    assert all(np.argmax(m[n]) == m[n].size - 1 for n in range(3))
    assert (O.colourise(m, "bone")[:, -1, -1] == bone[-1]).all()
    m = C.planted("equals_max_value")
    assert (O.colourise(m, "rainbow", 10)[:, 1, 2] == rainbow[-1]).all()
    m = C.planted("zero_disparity")
    depth = O.colourise(m, "rainbow", 10, True)
    assert (depth[1, 5, 7] == rainbow[-1]).all() and (depth[2, 0, 0] == rainbow[0]).all()
    m = C.planted("negative")
    assert (O.colourise(m, "bone")[0, 3, 4] == bone[0]).all()
    m = C.planted("nan_in_one_image")
    disp = O.colourise(m, "bone")
    assert not disp[1].any() and (disp[0][..., 3] == 255).all() and (disp[2][..., 3] == 255).all()
    clean = C.base((3, 37, 53), seed=1)
    assert np.array_equal(disp[[0, 2]], O.colourise(clean, "bone")[[0, 2]])
    assert np.isnan(O.image_max(m)[1]) and not np.isnan(O.image_max(m)[[0, 2]]).any()
    m = C.planted("all_zero_image")
    assert not O.colourise(m, "bone")[2].any() and O.colourise(m, "bone")[0].any()
    m = C.planted("mostly_far")
    assert ((1 / m[0]) > 10).mean() > 0.5
    assert (O.colourise(m, "rainbow", 10, True)[0] == rainbow[-1]).all(axis=-1).mean() > 0.5


def test_buffers_off_the_16_byte_boundary_take_the_scalar_path():
    maps = C.planted("nan_in_one_image")
    for offset in (4, 8):
        check_pictures(maps, lambda *a: H.colourise(*a, offset=offset))


def test_normalisation_on_every_byte_value():
    seen = set()
    for frames in C.all_bytes():
        got = H.normalise_u8(frames)
        want = O.normalise(frames)
        t = torch.from_numpy(frames.astype(np.float32)).permute(0, 3, 1, 2)
        torch_cpu = ((t / 255 - 0.45) / 0.225).contiguous().numpy()
        assert got.shape == (2, 3, 5, 7) and got.dtype == np.float32
        assert np.array_equal(got.view(np.uint32), torch_cpu.view(np.uint32))
        assert np.array_equal(want.view(np.uint32), torch_cpu.view(np.uint32))
        seen |= set(frames.ravel().tolist())
    assert seen == set(range(256))


def test_maximum_of_negative_images_and_zeros():
    maps = -C.base((3, 37, 53), seed=2) - np.float32(1e-3)
    maps[1, 3, 3] = -np.inf
    assert same_floats(H.image_max(maps), O.image_max(maps)) and (O.image_max(maps) < 0).all()
    zeros = np.zeros((2, 3, 5), np.float32)
    zeros[1, 0, 0] = -0.0
    assert same_floats(H.image_max(zeros), np.zeros(2, np.float32))
    big = C.base((1, 200, 300), seed=3)  # more pixels than one block of the maximum folds in one step
    big[0, 199, 299] = 7.0
    assert same_floats(H.image_max(big), np.array([7.0], np.float32))
