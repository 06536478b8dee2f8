"""scsfm_prep_resize_u8 on the host simulator equals PIL's Image.resize(BILINEAR) byte for byte."""
import numpy as np
import pytest

import _hostsim_prep as hs
from _prepare_data_check import RESIZE_CASES, pil_resize, resize_inputs
from scsfm_hip import prepare


@pytest.mark.parametrize("name", list(RESIZE_CASES))
def test_resize_equals_pil(name):
    images, h, w, keep = resize_inputs(name)
    got = hs.resize_u8(images, h, w, keep)
    assert got.shape == (len(images), keep or h, w, images.shape[3])
    assert np.array_equal(got, pil_resize(images, h, w, keep))


def test_tap_counts_and_source_rows():
    rows, taps = prepare.axis_table(61, 20)
    # more taps than the five of the bicubic up-scaling tables, at most Pillow's ksize = 2 ceil(support) + 1
    assert 5 < rows[:, 1].max() <= 9 and rows[0, 0] == 0 and rows[-1, 0] + rows[-1, 1] == 61
    assert len(taps) == rows[:, 1].sum() and rows[-1, 2] + rows[-1, 1] == len(taps)
    assert 9 < prepare.axis_table(205, 41)[0][:, 1].max() <= 11
    assert prepare.axis_table(13, 31)[0][:, 1].max() <= 3
    assert prepare.axis_table(12, 12) is None
    plan = prepare.resize_plan(59, 205, 12, 41, 9)
    # 9 of 12 output rows reach only the first source rows: the rest is not resampled horizontally
    assert plan["keep"] == 9 and plan["src_row0"] == 0 and plan["src_rows"] < 59
    with pytest.raises(ValueError):
        prepare.resize_plan(59, 205, 12, 41, 13)
