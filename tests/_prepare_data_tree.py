"""Miniature raw datasets for the tests of data/prepare_train_data.py: the KITTI-raw drive of the fixtures
(tests/golden/prepare_data.npz and tests/golden/prepare_data/*.txt) written out as a download would look, and generated
KITTI-odometry and Cityscapes trees.  Test infrastructure only."""
from __future__ import annotations

import json
import os

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
NPZ = os.path.join(GOLDEN, "prepare_data.npz")
TEXT = os.path.join(GOLDEN, "prepare_data")
TEST_SCENES = os.path.join(TEXT, "test_scenes.txt")
CALIB = ("calib_cam_to_cam.txt", "calib_velo_to_cam.txt", "calib_imu_to_velo.txt")

DATE = "2011_09_26"
DATES = ("2011_09_26", "2011_09_28", "2011_09_29", "2011_09_30", "2011_10_03")
DRIVE = DATE + "_drive_0001_sync"       # a training drive
TEST_DRIVE = DATE + "_drive_0002_sync"  # on the list of test scenes: must never be prepared
HEIGHT, WIDTH = 16, 48                  # the size the miniature drive is prepared at
RAW_H, RAW_W = 30, 100


def write_kitti_raw(root, frames, oxts, scans, calib_dir=TEXT, second_drive=False):
    """frames uint8 [n, H, W, 3], oxts float64 [n, 30], scans: list of float32 [m, 4] (frame k gets scan k % len)."""
    date = os.path.join(root, DATE)
    for other in DATES:  # (a download holds all five dates)
        os.makedirs(os.path.join(root, other), exist_ok=True)
    for name in CALIB:
        with open(os.path.join(calib_dir, name)) as f, open(os.path.join(date, name), "w") as g:
            g.write(f.read())
    drives = [DRIVE] + ([DATE + "_drive_0005_sync"] if second_drive else [])
    for drive in drives:
        for sub in ("oxts/data", "image_02/data", "image_03/data", "velodyne_points/data"):
            os.makedirs(os.path.join(date, drive, sub), exist_ok=True)
        for k, (img, row) in enumerate(zip(frames, oxts)):
            fid = "{:010d}".format(k)
            with open(os.path.join(date, drive, "oxts/data", fid + ".txt"), "w") as f:
                f.write(" ".join(repr(float(x)) for x in row) + "\n")
            Image.fromarray(img).save(os.path.join(date, drive, "image_02/data", fid + ".png"))
            Image.fromarray(img[:, ::-1].copy()).save(os.path.join(date, drive, "image_03/data", fid + ".png"))
            scans[k % len(scans)].astype(np.float32).tofile(os.path.join(date, drive, "velodyne_points/data", fid + ".bin"))
    os.makedirs(os.path.join(date, TEST_DRIVE, "oxts", "data"), exist_ok=True)
    return root


def fixture_tree(root, **kw):
    z = np.load(NPZ)
    return write_kitti_raw(root, z["frames"], z["oxts"], [z["scan0"], z["scan1"]], **kw)


def write_kitti_odom(root, seed=3):
    rng = np.random.default_rng(seed)
    for seq, n in (("00", 4), ("03", 3), ("09", 3)):  # 09 is a test sequence
        d = os.path.join(root, "sequences", seq)
        for cam in ("2", "3"):
            os.makedirs(os.path.join(d, "image_" + cam), exist_ok=True)
            for k in range(n):
                Image.fromarray(rng.integers(0, 256, (20, 64, 3), dtype=np.uint8)).save(
                    os.path.join(d, "image_" + cam, "{:06d}.png".format(k)))
        with open(os.path.join(d, "calib.txt"), "w") as f:
            for j in range(4):
                P = np.array([[718.856 + j, 0, 607.1928, -386.1448 * j], [0, 718.856 + j, 185.2157, 0.01 * j], [0, 0, 1, 0.003 * j]])
                f.write("P{}: ".format(j) + " ".join("%.12e" % x for x in P.ravel()) + "\n")
    return root


def write_cityscapes(root, seed=4):
    rng = np.random.default_rng(seed)
    # city -> scene -> frame numbers (two connected runs in the first scene) and speeds on both sides of the gate
    layout = {"aachen": {"000000": list(range(0, 9)) + list(range(12, 19)), "000001": list(range(5, 11))},
              "bonn": {"000003": list(range(2, 9))}}
    for city, scenes in layout.items():
        img_dir = os.path.join(root, "leftImg8bit_sequence", "train", city)
        cam_dir = os.path.join(root, "camera", "train", city)
        veh_dir = os.path.join(root, "vehicle_sequence", "train", city)
        for d in (img_dir, cam_dir, veh_dir):
            os.makedirs(d, exist_ok=True)
        for scene, ids in scenes.items():
            for n in ids:
                fid = "{:06d}".format(n)
                Image.fromarray(rng.integers(0, 256, (32, 64, 3), dtype=np.uint8)).save(
                    os.path.join(img_dir, "{}_{}_{}_leftImg8bit.png".format(city, scene, fid)))
                with open(os.path.join(veh_dir, "{}_{}_{}_vehicle.json".format(city, scene, fid)), "w") as f:
                    json.dump({"speed": float(rng.choice([0.3, 0.9, 1.4, 6.5])), "yawRate": 0.0}, f)
            with open(os.path.join(cam_dir, "{}_{}_{:06d}_camera.json".format(city, scene, ids[len(ids) // 2])), "w") as f:
                json.dump({"intrinsic": {"fx": 2262.52 + len(ids), "fy": 2265.3017905988554, "u0": 1096.98, "v0": 513.137}}, f)
    return root
