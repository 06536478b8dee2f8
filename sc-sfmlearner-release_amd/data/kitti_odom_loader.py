"""KITTI odometry for data/prepare_train_data.py: sequences 00-08, cameras 2 and 3, intrinsics from calib.txt.  As
data/kitti_raw_loader.py, the loader selects and describes; it decodes nothing."""
from __future__ import annotations

import glob
import os

import numpy as np

from kitti_raw_loader import image_size


class KittiOdomLoader:
    cam_ids = ["2", "3"]
    train_sets = ["00", "01", "02", "03", "04", "05", "06", "07", "08"]
    test_sets = ["09", "10"]

    def __init__(self, dataset_dir, img_height=256, img_width=832):
        self.dataset_dir = str(dataset_dir)
        self.img_height, self.img_width = img_height, img_width
        self.keep_rows = None
        self.scenes = [d for d in sorted(glob.glob(os.path.join(self.dataset_dir, "sequences", "*")))
                       if os.path.isdir(d) and os.path.basename(d) in self.train_sets]

    def image_file(self, scene, i):
        return os.path.join(scene["dir"], "image_" + scene["cid"], scene["frame_id"][i] + ".png")

    def collect_scenes(self, drive):
        scenes = []
        for cid in self.cam_ids:
            scene = {"cid": cid, "dir": drive, "rel_path": os.path.basename(drive) + "_" + cid}
            # (sorted: the order of a directory listing is the file system's own)
            scene["frame_id"] = sorted(f.split(".")[0] for f in os.listdir(os.path.join(drive, "image_" + cid)))
            if not scene["frame_id"] or not os.path.isfile(self.image_file(scene, 0)):
                return []
            h, w = image_size(self.image_file(scene, 0))
            scene["intrinsics"] = self.read_calib_file(cid, os.path.join(drive, "calib.txt"), self.img_width / w,
                                                       self.img_height / h)
            scenes.append(scene)
        return scenes

    def read_calib_file(self, cid, path, zoom_x, zoom_y):
        """The 3x3 of line P<cid> of calib.txt, kept in float32 as it is parsed, its rows scaled by the zoom."""
        with open(path) as f:
            lines = f.readlines()
        K = np.array(lines[int(cid)].split()[1:]).reshape(3, 4).astype(np.float32)[:3, :3]
        K[0, :] *= zoom_x
        K[1, :] *= zoom_y
        return K

    def frames(self, scene):
        return [{"id": fid, "img_file": self.image_file(scene, i)} for i, fid in enumerate(scene["frame_id"])]
