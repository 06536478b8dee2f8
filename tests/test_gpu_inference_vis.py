"""scsfm_hip.visualise on the GPU against the numpy oracle (tests/inference_vis_oracle.py): the pictures byte for byte,
the maxima and the normalisation bit for bit, on the shapes and planted values of tests/_inference_vis_cases.py, one
KITTI-sized batch, a non-contiguous input and a non-default stream."""
import numpy as np
import pytest
import torch

import _inference_vis_cases as C
import inference_vis_oracle as O
from scsfm_hip import visualise as V

pytestmark = pytest.mark.gpu


def same_floats(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


def check(maps, staged=None):
    staged = torch.from_numpy(maps).cuda() if staged is None else staged
    assert same_floats(V.image_max(staged).cpu().numpy(), O.image_max(maps))
    for name, max_value, reciprocal in C.CALLS:
        got = V.colourise(staged, name, max_value, reciprocal)
        assert got.is_cuda and got.dtype == torch.uint8 and got.shape == maps.shape + (4,)
        got = got.cpu().numpy()
        want = O.colourise(maps, name, max_value, reciprocal)
        bad = np.argwhere((got != want).any(axis=-1))
        assert len(bad) == 0, (name, max_value, reciprocal, len(bad), bad[:4].tolist())


@pytest.mark.parametrize("shape", C.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_pictures_on_every_shape(shape):
    check(C.base(shape))


@pytest.mark.parametrize("plant", list(C.PLANTS))
def test_planted_values(plant):
    check(C.planted(plant))


def test_kitti_sized_batch():
    maps = C.base((2, 256, 832), seed=5)
    maps[1] *= np.float32(0.05)  # the second image: depths beyond 10 nearly everywhere
    maps[0, 255, 831] = 3.0
    check(maps)


def test_non_contiguous_input_and_a_view_off_the_16_byte_boundary():
    wide = C.base((3, 37, 60), seed=6)
    staged = torch.from_numpy(wide).cuda()[:, :, 3:56]
    assert not staged.is_contiguous()
    check(np.ascontiguousarray(wide[:, :, 3:56]), staged)
    flat = torch.from_numpy(C.base((1, 1, 3 * 37 * 53 + 1), seed=8)).cuda()
    view = flat[0, 0, 1:].reshape(3, 37, 53)  # contiguous, 4 bytes past the boundary: the one-pixel-per-lane path
    assert view.is_contiguous() and view.data_ptr() % 16 == 4
    check(view.cpu().numpy(), view)


def test_non_default_stream():
    maps = C.planted("nan_in_one_image")
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        staged = torch.from_numpy(maps).cuda()
        disp, depth = V.disparity_and_depth_images(staged[:, None])
        first = V.colourise(staged, "bone")
    stream.synchronize()
    want_disp, want_depth = O.disparity_and_depth(maps)
    assert np.array_equal(disp.cpu().numpy(), want_disp) and np.array_equal(depth.cpu().numpy(), want_depth)
    assert torch.equal(first, disp)


def test_normalisation_equals_the_torch_cpu_expression():
    for frames in C.all_bytes() + [np.random.default_rng(1).integers(0, 256, (2, 64, 96, 3), dtype=np.uint8)]:
        got = V.normalise_u8(torch.from_numpy(frames).cuda())
        t = torch.from_numpy(frames.astype(np.float32)).permute(0, 3, 1, 2)
        want = ((t / 255 - 0.45) / 0.225).contiguous().numpy()
        assert got.shape == want.shape and got.dtype == torch.float32 and got.is_contiguous()
        assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))
        assert np.array_equal(O.normalise(frames).view(np.uint32), want.view(np.uint32))


def test_maximum_of_negative_images():
    maps = -C.base((3, 37, 53), seed=2) - np.float32(1e-3)
    maps[1, 3, 3] = -np.inf
    got = V.image_max(torch.from_numpy(maps).cuda())
    again = V.image_max(torch.from_numpy(maps).cuda())
    assert same_floats(got.cpu().numpy(), O.image_max(maps)) and torch.equal(got, again)
