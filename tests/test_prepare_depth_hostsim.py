"""scsfm_prep_velo_depth on the host simulator against the reference's generate_depth_map: the goldens, and the live
reference where its checkout exists."""
import os

import numpy as np
import pytest

import _hostsim_prep as hs
import _prepare_data_ref as R
import _prepare_data_tree as T
from _prepare_data_check import cloud, golden_depth_inputs, golden_projection, judge_depth


@pytest.mark.parametrize("ratio", [1, 2])
def test_golden_scans(ratio):
    points, off, P, h, w, bounds, want = golden_depth_inputs(ratio)
    got = hs.velodyne_depth(points, off, P, h, w, bounds)
    judge_depth(got, want, f"hostsim, golden scans, ratio {ratio}")


def test_the_constructed_cases():
    """Camera 02, ratio 1, scan 0 (tests/make_prepare_data_golden.py: build_scan0)."""
    points, off, P, h, w, bounds, _ = golden_depth_inputs(1)
    d = hs.velodyne_depth(points[:off[1]], off[:2], P[:1], h, w, bounds)[0]
    f = np.float32
    assert abs(d[5, 10] - f(7)) < 1e-5 and abs(d[9, 30] - f(4)) < 1e-5           # the minimum, not first, not last
    assert abs(d[3, w - 1] - f(11)) < 1e-5 and abs(d[4, 0] - f(11)) < 1e-5       # the false collision: 20 became 11
    assert abs(d[8, 0] - f(12)) < 1e-5 and abs(d[7, w - 1] - f(12)) < 1e-5       # ... and 21 became 12
    assert d[12, 20] == 0 and d[13, 33] == 0                                      # negative depth; behind the sensor
    assert d[h - 1, w - 1] > 0 and d[11, w - 1] > 0 and d[h - 1, 17] > 0


def test_empty_scan_gives_zeros():
    _, P = cloud(0, 6, 20, 0)
    d = hs.velodyne_depth(np.zeros((0, 4), np.float32), [0, 0], P[None], 6, 20, (20.0, 6.0))
    assert d.shape == (1, 6, 20) and not d.any()


@pytest.mark.skipif(not R.available(), reason="the reference checkout is not on this machine")
@pytest.mark.parametrize("ratio", [1, 2])
def test_live_reference(tmp_path, ratio):
    root = T.fixture_tree(str(tmp_path))
    data = os.path.join(root, T.DATE, T.DRIVE, "velodyne_points", "data")
    for cid in ("02", "03"):
        P, P_rect = golden_projection(cid, ratio)
        for k in (0, 1):
            f = os.path.join(data, "{:010d}.bin".format(k))
            want = R.depth_map(P_rect, f, os.path.join(root, T.DATE), T.HEIGHT, T.WIDTH, ratio)
            pts = np.fromfile(f, np.float32).reshape(-1, 4)
            got = hs.velodyne_depth(pts, [0, len(pts)], P[None], T.HEIGHT // ratio, T.WIDTH // ratio,
                                    (T.WIDTH / ratio, T.HEIGHT / ratio))[0]
            judge_depth(got, want, f"hostsim, live reference, camera {cid}, ratio {ratio}, scan {k}")
