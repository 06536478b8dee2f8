"""scsfm_hip.fusion's host-side pieces (no GPU): write_ply's file read back field by field, and bounds_from_cameras /
camera_box on hand-made poses."""
import numpy as np
import pytest
import torch

from scsfm_hip import fusion


def _pose(x, y, z):
    return np.concatenate([np.eye(3), [[x], [y], [z]]], axis=1)


def test_write_ply_round_trip(tmp_path):
    rng = np.random.default_rng(2)
    xyz = rng.standard_normal((7, 3)).astype(np.float32)
    xyz[3] = [np.float32(1e-30), -0.0, 3.5]
    rgb = rng.integers(0, 256, (7, 3)).astype(np.uint8)
    path = tmp_path / "points.ply"
    fusion.write_ply(str(path), torch.from_numpy(xyz), rgb)
    blob = path.read_bytes()
    head, body = blob.split(b"end_header\n", 1)
    assert head.decode("ascii").splitlines() == [
        "ply", "format binary_little_endian 1.0", "element vertex 7", "property float x", "property float y",
        "property float z", "property uchar red", "property uchar green", "property uchar blue"]
    assert len(body) == 7 * 15
    for k in range(7):
        row = body[15 * k:15 * k + 15]
        assert row[:12] == xyz[k].astype("<f4").tobytes() and list(row[12:]) == rgb[k].tolist()
    fusion.write_ply(str(path), np.zeros((0, 3), np.float32), np.zeros((0, 3), np.uint8))
    assert path.read_bytes().endswith(b"element vertex 0\nproperty float x\nproperty float y\nproperty float z\n"
                                      b"property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n")
    with pytest.raises(ValueError):
        fusion.write_ply(str(path), xyz, rgb[:5])
    with pytest.raises(ValueError):
        fusion.write_ply(str(path), xyz[:, :2], rgb[:, :2])


def test_bounds_from_cameras_on_hand_made_poses():
    c2w = np.stack([_pose(0, 0, 0), _pose(2.0, -0.5, 1.0), _pose(1.0, 0.25, 4.0)])
    lo, hi = fusion.camera_box(c2w, 3.0)
    assert lo.tolist() == [-3.0, -3.5, -3.0] and hi.tolist() == [5.0, 3.25, 7.0]
    origin, dims = fusion.bounds_from_cameras(c2w, 3.0, 0.5)
    assert origin == (-3.0, -3.5, -3.0) and dims == (16, 14, 20)      # 8 / 0.5, 6.75 / 0.5 rounded up, 10 / 0.5
    origin, dims = fusion.bounds_from_cameras(torch.from_numpy(c2w.reshape(3, 12)), 3.0, 0.3)
    assert dims == (27, 23, 34)                                       # 26.67, 22.5, 33.33: all rounded up
    assert all(o + d * 0.3 >= h for o, d, h in zip(origin, dims, hi))
    assert fusion.bounds_from_cameras(c2w[:1], 1.0, 0.25)[1] == (8, 8, 8)  # one camera: a cube of twice max_depth
    assert fusion.bounds_from_cameras(c2w[:1], 1.0, 0.1)[1] == (20, 20, 20)  # (2 / 0.1 is 20, not 21)
    for bad in (dict(voxel_size=0.0), dict(voxel_size=-1.0)):
        with pytest.raises(ValueError):
            fusion.bounds_from_cameras(c2w, 3.0, **bad)
    with pytest.raises(ValueError):
        fusion.camera_box(c2w, 0.0)
    with pytest.raises(ValueError):
        fusion.camera_box(np.zeros((0, 3, 4)), 1.0)
    nan = c2w.copy()
    nan[1, 0, 3] = np.nan
    with pytest.raises(ValueError):
        fusion.camera_box(nan, 1.0)
