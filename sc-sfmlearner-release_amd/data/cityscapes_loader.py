"""Cityscapes for data/prepare_train_data.py: every city of leftImg8bit_sequence/<split>, cut into connected
sub-sequences, each split into its even and its odd frames, gated by the vehicle's speed; intrinsics from the camera
JSON; the bottom quarter of every resized frame (the car's bonnet) is not kept.  As data/kitti_raw_loader.py, the
loader selects and describes; it decodes nothing."""
from __future__ import annotations

import glob
import json
import os

import numpy as np

from kitti_raw_loader import image_size


class cityscapes_loader:
    def __init__(self, dataset_dir, split="train", crop_bottom=True, img_height=171, img_width=416):
        self.dataset_dir = str(dataset_dir)
        self.split = split
        self.crop_bottom = crop_bottom
        self.img_height, self.img_width = img_height, img_width
        self.keep_rows = int(img_height * 0.75) if crop_bottom else None
        self.min_speed = 2
        self.scenes = [d for d in sorted(glob.glob(os.path.join(self.dataset_dir, "leftImg8bit_sequence", split, "*")))
                       if os.path.isdir(d)]
        print("Total scenes collected: {}".format(len(self.scenes)))

    def image_file(self, city, scene_id, frame_id):
        return os.path.join(city, "{}_{}_{}_leftImg8bit.png".format(os.path.basename(city), scene_id, frame_id))

    def collect_scenes(self, city):
        name = os.path.basename(city)
        by_scene = {}
        for f in sorted(glob.glob(os.path.join(city, "*.png"))):
            scene_id, frame_id = os.path.basename(f).split("_")[1:3]
            by_scene.setdefault(scene_id, []).append(frame_id)
        out = []
        for scene_id, ids in by_scene.items():
            # connected runs: a gap of more than one frame number starts a new one
            runs, previous = [], None
            for fid in ids:
                if previous is None or int(fid) - int(previous) > 1:
                    runs.append([])
                runs[-1].append(fid)
                previous = fid
            intrinsics = self.load_intrinsics(city, scene_id)
            for run in runs:
                speeds = [self.load_speed(city, scene_id, fid) for fid in run]
                for parity in (0, 1):
                    out.append({"city": city, "scene_id": scene_id, "intrinsics": intrinsics,
                                "rel_path": "{}_{}_{}_{}".format(name, scene_id, run[0], parity),
                                "frame_ids": run[parity::2], "speeds": speeds[parity::2]})
        return out

    def load_intrinsics(self, city, scene_id):
        name = os.path.basename(city)
        folder = os.path.join(self.dataset_dir, "camera", self.split, name)
        camera_file = sorted(glob.glob(os.path.join(folder, "{}_{}_*_camera.json".format(name, scene_id))))[0]
        frame_id = os.path.basename(camera_file).split("_")[2]
        with open(camera_file) as f:
            cam = json.load(f)["intrinsic"]
        K = np.array([[cam["fx"], 0, cam["u0"]], [0, cam["fy"], cam["v0"]], [0, 0, 1]])
        h, w = image_size(self.image_file(city, scene_id, frame_id))
        K[0] *= self.img_width / w
        K[1] *= self.img_height / h
        return K

    def load_speed(self, city, scene_id, frame_id):
        name = os.path.basename(city)
        path = os.path.join(self.dataset_dir, "vehicle_sequence", self.split, name,
                            "{}_{}_{}_vehicle.json".format(name, scene_id, frame_id))
        with open(path) as f:
            return json.load(f)["speed"]

    def frames(self, scene):
        out, cum = [], np.zeros(3)
        for fid, speed in zip(scene["frame_ids"], scene["speeds"]):
            cum += speed
            if np.linalg.norm(cum) > self.min_speed:
                out.append({"id": fid, "img_file": self.image_file(scene["city"], scene["scene_id"], fid)})
                cum *= 0
        return out
