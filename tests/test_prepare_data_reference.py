"""This repository's loaders against the reference's own, live, on miniature trees (KITTI raw, odometry, Cityscapes):
the same scenes, frames and rel_paths; intrinsics to 1e-12 relative; poses to 1e-9 in the rotation entries and 1e-6 m
in the translations (float64 rounding on 6.4e6 m Mercator coordinates through five 4x4 products is about 1e-8 m)."""
import os
import sys

import numpy as np
import pytest

import _prepare_data_ref as R
import _prepare_data_tree as T

DATA = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "sc-sfmlearner-release_amd", "data")
if DATA not in sys.path:
    sys.path.insert(0, DATA)

pytestmark = pytest.mark.skipif(not R.available(), reason="the reference checkout is not on this machine")


def describe(loader):
    out = []
    for drive in loader.scenes:
        for scene in loader.collect_scenes(drive):
            frames = loader.frames(scene)
            rec = {"rel_path": scene["rel_path"], "intrinsics": np.array(scene["intrinsics"]),
                   "ids": [f["id"] for f in frames]}
            if frames and "pose" in frames[0]:
                rec["poses"] = np.array([f["pose"] for f in frames])
            out.append(rec)
    return out


def same_scenes(ours, ref, sort_ids=False):
    assert len(ours) == len(ref) > 0
    assert [s["rel_path"] for s in ours] == [s["rel_path"] for s in ref]
    for a, b in zip(ours, ref):
        assert a["ids"] == (sorted(b["ids"]) if sort_ids else b["ids"]), a["rel_path"]
        assert a["intrinsics"].shape == b["intrinsics"].shape == (3, 3) and a["intrinsics"].dtype == b["intrinsics"].dtype
        assert np.allclose(a["intrinsics"], b["intrinsics"], rtol=1e-12, atol=0), a["rel_path"]


def same_poses(ours, ref):
    for a, b in zip(ours, ref):
        assert a["poses"].shape == b["poses"].shape and a["poses"].shape[1:] == (3, 4)
        assert np.abs(a["poses"][:, :, :3] - b["poses"][:, :, :3]).max() <= 1e-9
        assert np.abs(a["poses"][:, :, 3] - b["poses"][:, :, 3]).max() <= 1e-6


@pytest.mark.parametrize("static", [False, True])
def test_kitti_raw(tmp_path, static):
    from kitti_raw_loader import KittiRawLoader
    root = T.fixture_tree(str(tmp_path / "raw"), second_drive=True)
    static_file = None
    if static:
        static_file = str(tmp_path / "static.txt")
        with open(static_file, "w") as f:
            f.write("2011_09_26 2011_09_26_drive_0001_sync 0000000001\n2011_09_26 2011_09_26_drive_0001_sync 0000000004\n\n"
                    "2011_09_26 2011_09_26_drive_0005_sync 0000000000\n")
    scenes = [ln.strip() for ln in open(T.TEST_SCENES)]
    ours = describe(KittiRawLoader(root, scenes, static_frames_file=static_file, img_height=T.HEIGHT, img_width=T.WIDTH,
                                   get_pose=True))
    ref = R.kitti_raw(root, T.HEIGHT, T.WIDTH, static_frames_file=static_file, get_pose=True)
    assert len(ours) == 4 and not any("0002" in s["rel_path"] for s in ours)  # two drives x two cameras; no test drive
    same_scenes(ours, ref)
    same_poses(ours, ref)
    assert len(ours[0]["ids"]) == (6 if static else 4) and len(ours[2]["ids"]) == (7 if static else 4)


def test_kitti_raw_matches_the_goldens(tmp_path):
    from kitti_raw_loader import KittiRawLoader
    z = np.load(T.NPZ)
    root = T.fixture_tree(str(tmp_path))
    ours = describe(KittiRawLoader(root, [ln.strip() for ln in open(T.TEST_SCENES)], img_height=T.HEIGHT,
                                   img_width=T.WIDTH, get_pose=True))
    assert [s["rel_path"] for s in ours] == list(z["rel_paths"]) and ours[0]["ids"] == list(z["ids"])
    assert np.allclose(np.array([s["intrinsics"] for s in ours]), z["intrinsics"], rtol=1e-12, atol=0)
    same_poses(ours, [{"poses": p} for p in z["poses"]])


def test_kitti_odometry(tmp_path):
    from kitti_odom_loader import KittiOdomLoader
    root = T.write_kitti_odom(str(tmp_path))
    ours = describe(KittiOdomLoader(root, img_height=10, img_width=32))
    ref = R.kitti_odom(root, 10, 32)
    assert len(ours) == 4  # sequences 00 and 03, cameras 2 and 3; 09 is for testing
    # (the reference lists a folder's frames in the file system's order; here they are sorted)
    same_scenes(ours, ref, sort_ids=True)


def test_cityscapes(tmp_path_factory):
    from cityscapes_loader import cityscapes_loader
    # (a folder without '_' in its name: the reference takes the frame id of a camera file from the third '_'-separated
    # piece of its whole path)
    root = T.write_cityscapes(str(tmp_path_factory.mktemp("cs")))
    if "_" in os.path.dirname(root):
        pytest.skip("the temporary folder's path holds an underscore, which the reference's loader cannot take")
    loader = cityscapes_loader(root, img_height=16, img_width=32)
    assert loader.keep_rows == 12
    ours = describe(loader)
    ref = R.cityscapes(root, 16, 32)
    assert len(ours) == 8  # (2 runs + 1 run) + 1 run, each split into even and odd frames
    same_scenes(ours, ref)
    assert any(s["ids"] for s in ours) and any(len(s["ids"]) < 4 for s in ours)
    assert all(img.shape == (12, 32, 3) for s in ref for img in s["imgs"])
