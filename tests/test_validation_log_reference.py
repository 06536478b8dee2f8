"""scsfm_hip.validation_log's tables and the numpy restatement (tests/validation_log_oracle.py) against the reference's
own utils.py and train.py statements run live (tests/_validation_log_ref.py; skipped when the reference or matplotlib is
absent), and the golden file against what the reference gives now.  Entry for entry, bit for bit."""
import os

import numpy as np
import pytest

import _inference_vis_cases as C
import _validation_log_golden as G
import _validation_log_ref as R
import validation_log_oracle as O
from scsfm_hip import validation_log as VL

needs_reference = pytest.mark.skipif(not R.available(), reason="the reference (or matplotlib) is not on this machine")


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


@pytest.mark.parametrize("name,n", [("rainbow", 1000), ("magma", 1000), ("bone", 10000)])
def test_tables_equal_the_golden_at_every_entry(name, n):
    table = VL.colour_table_f32(name)
    assert table.shape == (n, 4) and table.dtype == np.float32 and not table.flags.writeable
    assert same(table, G.load()[name])
    assert (table[:, 3] == 1).all() and table.min() >= 0 and table.max() <= 1
    assert VL.colour_table_f32(name) is table  # cached


def test_golden_is_small():
    assert os.path.getsize(G.PATH) < 100 * 1024


@needs_reference
@pytest.mark.parametrize("name", R.NAMES)
def test_tables_equal_the_live_reference(name):
    assert same(VL.colour_table_f32(name), R.float_table(name))


@needs_reference
def test_magma_list_equals_the_installed_matplotlib():
    mine = np.array(VL._MAGMA_MILLIONTHS.split(), dtype=np.float64).reshape(256, 3) / 1e6
    assert same(mine, R.magma_list())


@needs_reference
def test_golden_is_what_the_reference_gives_now():
    g = G.load()
    for key in "abc":
        for cmap, max_value in G.CALLS:
            assert same(R.map_pictures(g[f"maps_{key}"], max_value, cmap), g[f"{key}/{cmap}"]), (key, cmap)
    assert same(R.input_pictures(g["batch"]), g["batch/floats"])
    depth_pics, disps, disp_pics = R.target(g["gt"])
    assert same(depth_pics, g["gt/depth_picture"]) and same(disps, g["gt/disparity"])
    assert same(disp_pics, g["gt/disparity_picture"])


@needs_reference
@pytest.mark.parametrize("plant", list(C.PLANTS))
def test_oracle_equals_the_live_reference_on_the_planted_maps(plant):
    """The 37 x 53 maps of the inference pictures' tests, one planted value each, in both colour maps of train.py."""
    maps = C.planted(plant)
    for cmap, max_value in (("magma", None), ("rainbow", 10), ("magma", 10), ("rainbow", None)):
        want = R.map_pictures(maps, max_value, cmap)
        assert want.shape == (3, 4, 37, 53) and want.dtype == np.float32
        assert same(O.map_pictures(maps, VL.colour_table_f32(cmap), max_value), want), (cmap, max_value)
