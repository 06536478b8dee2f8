"""The numpy oracle (tests/inference_vis_oracle.py) against the reference's own utils.py run live
(tests/_inference_vis_ref.py; skipped when the reference or matplotlib is absent) and against what it recorded in
tests/golden/inference_vis.npz: both byte tables at every entry, both pictures, and the normalisation against the torch
CPU expression.  Byte for byte, bit for bit."""
import os

import numpy as np
import pytest
import torch

import _inference_vis_cases as C
import _inference_vis_ref as R
import inference_vis_oracle as O
from scsfm_hip import visualise

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "inference_vis.npz")
needs_reference = pytest.mark.skipif(not R.available(), reason="the reference (or matplotlib) is not on this machine")


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.mark.parametrize("name,n", [("bone", 10000), ("rainbow", 1000)])
def test_tables_equal_the_golden_at_every_entry(golden, name, n):
    assert golden[name].shape == (n, 4)
    assert np.array_equal(O.table(name), golden[name])
    assert np.array_equal(visualise.colour_table(name), golden[name])
    assert (golden[name][:, 3] == 255).all()


def test_pictures_equal_the_golden(golden):
    disp = golden["disp"]
    got_disp, got_depth = O.disparity_and_depth(disp)
    assert np.array_equal(got_disp, golden["disp_pictures"])
    assert np.array_equal(got_depth, golden["depth_pictures"])
    # what the six maps were chosen for
    assert np.isnan(disp[3]).sum() == 1 and not golden["disp_pictures"][3].any() and not golden["disp_pictures"][4].any()
    assert (golden["depth_pictures"][2, 5, 7] == golden["rainbow"][-1]).all()
    assert (golden["depth_pictures"][5] == golden["rainbow"][-1]).all(axis=-1).mean() > 0.5
    assert (golden["disp_pictures"][1, -1, -1] == golden["bone"][-1]).all()


def test_golden_is_small():
    assert os.path.getsize(GOLDEN) < 100 * 1024


@needs_reference
@pytest.mark.parametrize("name", ["bone", "rainbow"])
def test_tables_equal_the_live_reference(name):
    assert np.array_equal(O.table(name), R.byte_table(name))


@needs_reference
def test_golden_is_what_the_reference_gives_now(golden):
    for i, d in enumerate(golden["disp"]):
        a, b = R.pictures(d[None])
        assert np.array_equal(a, golden["disp_pictures"][i]) and np.array_equal(b, golden["depth_pictures"][i]), i


@needs_reference
@pytest.mark.parametrize("plant", list(C.PLANTS))
def test_pictures_equal_the_live_reference(plant):
    maps = C.planted(plant)
    want = [R.pictures(m[None]) for m in maps]
    got_disp, got_depth = O.disparity_and_depth(maps)
    assert got_disp.shape == (3, 37, 53, 4)
    assert np.array_equal(got_disp, np.stack([w[0] for w in want]))
    assert np.array_equal(got_depth, np.stack([w[1] for w in want]))


@needs_reference
def test_fixed_divisor_without_reciprocal_equals_the_live_reference():
    """CALLS[2] of the cases: tensor2array(map, max_value=10, 'rainbow'), with a pixel at xa == N."""
    maps = C.planted("equals_max_value")
    U = R.utils()
    want = np.stack([(255 * U.tensor2array(torch.from_numpy(m[None]), max_value=10, colormap='rainbow')).astype(np.uint8)
                     .transpose(1, 2, 0) for m in maps])
    assert np.array_equal(O.colourise(maps, "rainbow", 10), want)


def test_normalisation_equals_the_torch_cpu_expression():
    for frames in C.all_bytes() + [np.random.default_rng(0).integers(0, 256, (2, 9, 11, 3), dtype=np.uint8)]:
        t = torch.from_numpy(frames.astype(np.float32)).permute(0, 3, 1, 2)
        want = ((t / 255 - 0.45) / 0.225).contiguous().numpy()
        assert np.array_equal(O.normalise(frames).view(np.uint32), want.view(np.uint32))
