"""KITTI raw for data/prepare_train_data.py: which drives, which frames, and the host-side metadata (numpy float64).

A loader here selects and describes; it decodes nothing.  ``collect_scenes(drive)`` gives one record per camera with
the intrinsics and, when asked, the poses; ``frames(scene)`` lists the chosen frames as records of file names.  The
pixels and the Velodyne scans go through scsfm_hip.prepare in the command-line program.
"""
from __future__ import annotations

import glob
import os

import numpy as np
from PIL import Image

from scsfm_hip.prepare import depth_map_size, velo_projection

EARTH_RADIUS = 6378137.0  # metres


def read_calib(path):
    """A KITTI calibration file as {key: float64 array}; lines that are not numbers (the dates) are left out."""
    data = {}
    with open(path) as f:
        for line in f:
            if ":" not in line:
                continue
            key, value = line.split(":", 1)
            try:
                data[key] = np.array([float(x) for x in value.split()])
            except ValueError:
                pass
    return data


def rigid(R, t):
    """4x4 from a rotation (9 numbers) and a translation (3 numbers)."""
    T = np.eye(4)
    T[:3, :3] = np.reshape(R, (3, 3))
    T[:3, 3] = np.reshape(t, 3)
    return T


def oxts_pose(lat, lon, alt, roll, pitch, yaw, scale):
    """The 4x4 pose of an OXTS packet: a Mercator-style projection with the scale of the drive's first frame for the
    translation, R = Rz(yaw) Ry(pitch) Rx(roll) for the rotation."""
    t = np.array([scale * lon * np.pi * EARTH_RADIUS / 180.0, lat * np.pi * EARTH_RADIUS / 180.0, alt])
    cx, sx, cy, sy, cz, sz = np.cos(roll), np.sin(roll), np.cos(pitch), np.sin(pitch), np.cos(yaw), np.sin(yaw)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return rigid(Rz.dot(Ry.dot(Rx)), t)


def image_size(path):
    """(height, width) from the file's header, without decoding it."""
    with Image.open(path) as im:
        return im.size[1], im.size[0]


def read_static_frames(path):
    """{drive: [ten-digit frame ids]} from lines of 'date drive frame'."""
    static = {}
    with open(path) as f:
        for line in f:
            if not line.strip():
                continue
            _, drive, frame = line.split()
            static.setdefault(drive, []).append("%.10d" % int(frame))
    return static


class KittiRawLoader:
    cam_ids = ["02", "03"]
    date_list = ["2011_09_26", "2011_09_28", "2011_09_29", "2011_09_30", "2011_10_03"]

    def __init__(self, dataset_dir, test_scenes, static_frames_file=None, img_height=128, img_width=416, min_speed=2,
                 get_depth=False, get_pose=False, depth_size_ratio=1):
        self.dataset_dir = str(dataset_dir)
        self.test_scenes = list(test_scenes)
        self.from_speed = static_frames_file is None
        self.static_frames = {} if self.from_speed else read_static_frames(static_frames_file)
        self.img_height, self.img_width = img_height, img_width
        self.min_speed = min_speed
        self.get_depth, self.get_pose = get_depth, get_pose
        self.depth_size_ratio = depth_size_ratio
        self.keep_rows = None
        if get_depth:
            self.depth_size = depth_map_size(img_height, img_width, depth_size_ratio)
        self.scenes = []
        for date in self.date_list:
            for drive in sorted(glob.glob(os.path.join(self.dataset_dir, date, "*"))):
                # (a drive is '<date>_drive_<number>_sync'; the list names it without '_sync')
                if os.path.isdir(drive) and os.path.basename(drive)[:-5] not in self.test_scenes:
                    self.scenes.append(drive)

    def image_file(self, scene, i):
        return os.path.join(scene["dir"], "image_" + scene["cid"], "data", scene["frame_id"][i] + ".png")

    def collect_scenes(self, drive):
        name, calib_dir = os.path.basename(drive), os.path.dirname(drive)
        imu2velo = read_calib(os.path.join(calib_dir, "calib_imu_to_velo.txt"))
        velo2cam = read_calib(os.path.join(calib_dir, "calib_velo_to_cam.txt"))
        cam2cam = read_calib(os.path.join(calib_dir, "calib_cam_to_cam.txt"))
        imu2cam = rigid(cam2cam["R_rect_00"], np.zeros(3)) @ rigid(velo2cam["R"], velo2cam["T"]) @ \
            rigid(imu2velo["R"], imu2velo["T"])
        cam2imu = np.linalg.inv(imu2cam)
        packets = [np.genfromtxt(f) for f in sorted(glob.glob(os.path.join(drive, "oxts", "data", "*.txt")))]
        scenes = []
        for cid in self.cam_ids:
            scene = {"cid": cid, "dir": drive, "rel_path": name + "_" + cid, "speed": [], "frame_id": [], "pose": []}
            scale = origin_inv = None
            for n, packet in enumerate(packets):
                scene["speed"].append(packet[8:11])
                scene["frame_id"].append("{:010d}".format(n))
                if scale is None:
                    scale = np.cos(packet[0] * np.pi / 180.0)
                pose = oxts_pose(*packet[:6], scale)
                if origin_inv is None:
                    origin_inv = np.linalg.inv(pose)
                scene["pose"].append((imu2cam @ origin_inv @ pose @ cam2imu)[:3])
            if not scene["frame_id"] or not os.path.isfile(self.image_file(scene, 0)):
                return []
            h, w = image_size(self.image_file(scene, 0))
            zoom_y, zoom_x = self.img_height / h, self.img_width / w
            P_rect = np.reshape(cam2cam["P_rect_" + cid], (3, 4)).copy()
            P_rect[0] *= zoom_x
            P_rect[1] *= zoom_y
            scene["P_rect"] = P_rect
            scene["intrinsics"] = P_rect[:, :3]
            if self.get_depth:
                scene["P_velo2im"] = velo_projection(P_rect, cam2cam["R_rect_00"], velo2cam["R"], velo2cam["T"],
                                                     self.depth_size_ratio)
            scenes.append(scene)
        return scenes

    def selected(self, scene):
        """Indices of the frames to keep: those at which the accumulated speed exceeds min_speed (the sum starts
        again there), or every frame that the static-frames list does not name."""
        if self.from_speed:
            keep, cum = [], np.zeros(3)
            for i, speed in enumerate(scene["speed"]):
                cum += speed
                if np.linalg.norm(cum) > self.min_speed:
                    keep.append(i)
                    cum *= 0
            return keep
        static = self.static_frames.get(os.path.basename(scene["dir"]), [])
        return [i for i, fid in enumerate(scene["frame_id"]) if fid not in static]

    def frames(self, scene):
        out = []
        for i in self.selected(scene):
            fid = scene["frame_id"][i]
            rec = {"id": fid, "img_file": self.image_file(scene, i)}
            if self.get_depth:
                rec["velo_file"] = os.path.join(scene["dir"], "velodyne_points", "data", fid + ".bin")
            if self.get_pose:
                rec["pose"] = scene["pose"][i]
            out.append(rec)
        return out
