"""Writes the fixtures of the prepare_train_data tests: tests/golden/prepare_data.npz and tests/golden/prepare_data/*.txt.

    python tests/make_prepare_data_golden.py          (by hand, where the reference checkout exists)

A generated miniature KITTI-raw drive (three calibration files, 8 OXTS packets with speeds on both sides of the
threshold, two Velodyne scans, random frames) and what the reference's own KittiRawLoader makes of it
(tests/_prepare_data_ref.py): the selected frame ids, intrinsics, poses, depth maps at ratio 1 and 2 and resized
frames.  test_scenes.txt is the reference's list of test drives, copied as data.

Scan 0 is built by back-projecting chosen (u, v, depth) through the calibration of camera 02 in float64 and rounding
to float32; the cases it holds are listed in build_scan0.  The script asserts that no projected coordinate of any
scan, camera and ratio lies within 1e-6 of a rounding tie, so that the reference's BLAS product and a left-to-right
sum cannot round a pixel differently."""
from __future__ import annotations

import os
import shutil
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, os.path.join(ROOT, "sc-sfmlearner-release_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import _prepare_data_ref as R  # noqa: E402
import _prepare_data_tree as T  # noqa: E402
from scsfm_hip.prepare import velo_projection  # noqa: E402

H, W = T.HEIGHT, T.WIDTH


def rot(rx, ry, rz):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    return np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @ \
        np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])


def line(key, values):
    return key + ": " + " ".join("%.12e" % v for v in np.ravel(values)) + "\n"


def write_calib(out):
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "calib_cam_to_cam.txt"), "w") as f:
        f.write("calib_time: 09-Jan-2012 13:57:47\n")
        f.write(line("R_rect_00", rot(0.004, -0.011, 0.007)))
        f.write(line("P_rect_02", [[70.0, 0, 50.5, 4.5], [0, 70.0, 15.25, 0.02], [0, 0, 1, 0.003]]))
        f.write(line("P_rect_03", [[70.0, 0, 50.5, -33.0], [0, 70.0, 15.25, 0.2], [0, 0, 1, 0.002]]))
    with open(os.path.join(out, "calib_velo_to_cam.txt"), "w") as f:
        f.write("calib_time: 15-Mar-2012 11:37:16\n")
        f.write(line("R", rot(0.002, -0.003, 0.005) @ np.array([[0.0, -1, 0], [0, 0, -1], [1, 0, 0]])))
        f.write(line("T", [-0.004, -0.076, -0.272]))
    with open(os.path.join(out, "calib_imu_to_velo.txt"), "w") as f:
        f.write("calib_time: 25-May-2012 16:47:16\n")
        f.write(line("R", rot(-0.001, 0.002, 0.0148)))
        f.write(line("T", [-0.8087, 0.3196, -0.7997]))


def read_calib(path):
    out = {}
    for ln in open(path):
        k, v = ln.split(":", 1)
        try:
            out[k] = np.array([float(x) for x in v.split()])
        except ValueError:
            pass
    return out


def projection(calib_dir, cid, ratio):
    """P_velo2im of the miniature drive (raw frames RAW_H x RAW_W prepared at H x W)."""
    c2c = read_calib(os.path.join(calib_dir, "calib_cam_to_cam.txt"))
    v2c = read_calib(os.path.join(calib_dir, "calib_velo_to_cam.txt"))
    P_rect = c2c["P_rect_" + cid].reshape(3, 4).copy()
    P_rect[0] *= W / T.RAW_W
    P_rect[1] *= H / T.RAW_H
    return velo_projection(P_rect, c2c["R_rect_00"], v2c["R"], v2c["T"], ratio)


def back_project(P, u, v, z, frac=0.2):
    """The velodyne point that projects to the unrounded coordinates (u + 1 + frac, v + 1 + frac) at depth z."""
    rhs = z * np.array([u + 1 + frac, v + 1 + frac, 1.0]) - P[:, 3]
    return np.concatenate([np.linalg.solve(P[:, :3], rhs), [0.5]])


def build_scan0(P, rng):
    """(u, v, depth) in index order.  Cases:
       three points on pixel (10, 5) with the minimum in the middle, and four on (30, 9) with it second;
       the false collision, column W - 1 of a row and column 0 of the next, in both index orders: rows 3 / 4 with
       the last column first, rows 7 / 8 with the first column first, the later point the nearer one in both;
       a point with negative camera depth (and forward x >= 0) on the otherwise empty pixel (20, 12);
       a point behind the sensor (x < 0) aimed at the otherwise empty pixel (33, 13);
       one point off each border; a point on (W - 1, H - 1); a point on column W - 1 alone and on row H - 1 alone."""
    pts = [(10, 5, 9.0), (2, 2, 14.0), (10, 5, 7.0), (W - 1, 3, 20.0), (10, 5, 8.0), (0, 4, 11.0),
           (0, 8, 21.0), (30, 9, 6.0), (30, 9, 4.0), (W - 1, 7, 12.0), (30, 9, 5.0), (30, 9, 4.5),
           (20, 12, -0.1), (33, 13, -3.0), (-3, 6, 10.0), (W + 1, 6, 10.0), (12, -2, 10.0), (12, H + 2, 10.0),
           (W - 1, H - 1, 13.0), (W - 1, 11, 15.0), (17, H - 1, 16.0)]
    taken = {(u, v) for u, v, _ in pts} | {(0, 4), (0, 8), (W - 1, 3), (W - 1, 7)}
    for _ in range(150):  # filler that stays off the pixels of the cases (it may collide with itself)
        u, v = int(rng.integers(0, W)), int(rng.integers(0, H))
        if (u, v) not in taken and (u, v) not in ((20, 12), (33, 13)):
            pts.append((u, v, float(rng.uniform(3, 40))))
    return np.array([back_project(P, *p, frac=rng.uniform(-0.3, 0.3)) for p in pts], dtype=np.float32)


def build_scan1(rng, n=300):
    return np.stack([rng.uniform(-4, 40, n), rng.uniform(-12, 12, n), rng.uniform(-2.5, 3, n), rng.uniform(0, 1, n)],
                    1).astype(np.float32)


def assert_no_ties(calib_dir, scans):
    for cid in ("02", "03"):
        for ratio in (1, 2):
            P = projection(calib_dir, cid, ratio)
            for s in scans:
                v = s.astype(np.float64).copy()
                v[:, 3] = 1
                q = v[v[:, 0] >= 0] @ P.T
                c = q[:, :2] / q[:, 2:]
                c = c[np.isfinite(c).all(1) & (np.abs(c) < 1e4).all(1)]
                dist = np.abs(np.abs(c - np.floor(c)) - 0.5)
                assert dist.min() > 1e-6, (cid, ratio, dist.min())


def main():
    assert R.available(), "the reference checkout is needed to write the fixtures"
    rng = np.random.default_rng(20240)
    write_calib(T.TEXT)
    shutil.copyfile(os.path.join(R.DATA, "test_scenes.txt"), T.TEST_SCENES)
    listed = [ln.strip() for ln in open(T.TEST_SCENES)]
    assert T.DRIVE[:-5] not in listed and T.TEST_DRIVE[:-5] in listed

    frames = rng.integers(0, 256, (8, T.RAW_H, T.RAW_W, 3), dtype=np.uint8)
    oxts = np.zeros((8, 30))
    oxts[:, 0] = 49.015 + 2e-6 * np.arange(8)
    oxts[:, 1] = 8.4339 + 3e-6 * np.arange(8) ** 1.5
    oxts[:, 2] = 116.4 + 0.05 * np.arange(8)
    oxts[:, 3:6] = np.stack([0.03 * np.sin(np.arange(8)), 0.01 * np.cos(np.arange(8)), -0.35 + 0.02 * np.arange(8)], 1)
    oxts[:, 8] = [0.5, 0.8, 1.2, 3.0, 0.1, 0.2, 2.5, 5.0]   # forward speed: frames 2, 3, 6 and 7 pass the gate
    oxts[:, 9] = [0.0, 0.1, -0.1, 0.2, 0.0, 0.05, 0.1, -0.2]
    scans = [build_scan0(projection(T.TEXT, "02", 1), rng), build_scan1(rng)]
    assert_no_ties(T.TEXT, scans)

    tmp = tempfile.mkdtemp(prefix="prepare_data_golden_")
    try:
        T.write_kitti_raw(tmp, frames, oxts, scans)
        r1 = R.kitti_raw(tmp, H, W, get_depth=True, get_pose=True, depth_size_ratio=1)
        r2 = R.kitti_raw(tmp, H, W, get_depth=True, get_pose=True, depth_size_ratio=2)
    finally:
        shutil.rmtree(tmp)
    assert [s["rel_path"] for s in r1] == [T.DRIVE + "_02", T.DRIVE + "_03"]
    assert r1[0]["ids"] == r1[1]["ids"] == ["{:010d}".format(k) for k in (2, 3, 6, 7)]
    d = r1[0]["depths"][0]  # camera 02, ratio 1, scan 0: the cases
    assert d[5, 10] == np.float32(7.0) or abs(d[5, 10] - 7.0) < 1e-4
    assert d[12, 20] == 0 and d[13, 33] == 0 and d[H - 1, W - 1] > 0 and d[11, W - 1] > 0 and d[H - 1, 17] > 0
    np.savez_compressed(
        T.NPZ, frames=frames, oxts=oxts, scan0=scans[0], scan1=scans[1], ids=np.array(r1[0]["ids"]),
        rel_paths=np.array([s["rel_path"] for s in r1]), intrinsics=np.array([s["intrinsics"] for s in r1]),
        poses=np.array([s["poses"] for s in r1]), depth_r1=np.array([s["depths"] for s in r1]),
        depth_r2=np.array([s["depths"] for s in r2]), imgs=np.array([s["imgs"] for s in r1]))
    print(T.NPZ, os.path.getsize(T.NPZ), "bytes; depth entries > 0:", int((r1[0]["depths"] > 0).sum()))
    print("false collision rows 3/4:", d[3, W - 1], d[4, 0], "rows 7/8:", d[7, W - 1], d[8, 0], "(30, 9):", d[9, 30])


if __name__ == "__main__":
    main()
