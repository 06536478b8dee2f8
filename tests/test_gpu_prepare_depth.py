"""scsfm_hip.prepare.velodyne_depth on the GPU: the golden scans against the reference's maps, generated clouds against
the host simulator (the same source in float64: bit-identical), batches of unequal scans, and two launches."""
import numpy as np
import pytest
import torch

import _hostsim_prep as hs
from _prepare_data_check import cloud, golden_depth_inputs, judge_depth
from scsfm_hip import prepare

pytestmark = pytest.mark.gpu


def on_gpu(points, off, P, h, w, bounds):
    args = (torch.from_numpy(np.ascontiguousarray(points, np.float32).reshape(-1, 4)).cuda(),
            torch.from_numpy(np.asarray(off, np.int32)).cuda(), torch.from_numpy(np.asarray(P, np.float64)).cuda())
    first = prepare.velodyne_depth(*args, h, w, bounds)
    second = prepare.velodyne_depth(*args, h, w, bounds)
    torch.cuda.synchronize()
    assert torch.equal(first.view(torch.int32), second.view(torch.int32))
    return first.cpu().numpy()


@pytest.mark.parametrize("ratio", [1, 2])
def test_golden_scans(ratio):
    points, off, P, h, w, bounds, want = golden_depth_inputs(ratio)
    judge_depth(on_gpu(points, off, P, h, w, bounds), want, f"gpu, golden scans, ratio {ratio}")


@pytest.mark.parametrize("n,h,w", [(0, 6, 20), (1, 6, 20), (257, 6, 20), (5000, 6, 20), (120000, 128, 416)])
def test_generated_cloud_equals_the_simulator(n, h, w):
    pts, P = cloud(n, h, w, seed=n + 1)
    if n == 1:
        pts[0] = (10.0, 0.5, 0.1, 0.3)  # in front of the camera, inside the map
    got = on_gpu(pts, [0, n], P[None], h, w, (float(w), float(h)))
    want = hs.velodyne_depth(pts, [0, n], P[None], h, w, (float(w), float(h)))
    assert np.array_equal(got.view(np.int32), want.view(np.int32))
    if n == 0:
        assert not got.any()
    if n == 1:
        assert (got > 0).sum() == 1
    if n == 5000:
        # 5,000 points for 120 pixels: every pixel that is hit is contended (a pixel whose nearest point has a
        # negative depth reads 0)
        assert (got > 0).sum() > h * w // 2


def test_batch_of_unequal_scans_with_an_empty_one():
    h, w = 12, 40
    a, P = cloud(700, h, w, seed=11)
    b, _ = cloud(333, h, w, seed=12)
    pts = np.concatenate([a, b])
    off = [0, 700, 700, 1033]
    Ps = np.stack([P, P * 1.0, P])
    got = on_gpu(pts, off, Ps, h, w, (float(w), float(h)))
    assert not got[1].any()
    for k, part in ((0, a), (2, b)):
        alone = hs.velodyne_depth(part, [0, len(part)], P[None], h, w, (float(w), float(h)))[0]
        assert np.array_equal(got[k].view(np.int32), alone.view(np.int32))
