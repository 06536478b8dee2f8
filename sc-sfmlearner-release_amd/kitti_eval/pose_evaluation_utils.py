"""The reference's kitti_eval/pose_evaluation_utils.py for users who import it: read_scene_data lists a KITTI odometry
tree's images, poses and snippet indices, and test_framework_KITTI yields one snippet after the other (images as float32
arrays, the ground-truth poses compensated by the first frame).  Written with os, glob and PIL (the reference needs
``path`` and ``imageio``).  test_pose.py takes only the file lists and the poses from here: its snippets are scored on
the GPU (scsfm_hip.snippets).

Two things differ from the reference.  The sequences come in sorted order (the reference iterates a ``set``, whose order
changes from run to run), and len(framework) is the number of snippets (the reference returns the number of images,
seq_length - 1 more per sequence than it yields).  ``img_exts`` is an addition; its default globs what the reference
globs."""
import glob
import os

import numpy as np


class test_framework_KITTI(object):
    def __init__(self, root, sequence_set, seq_length=3, step=1, img_exts=("png",)):
        self.root = root
        scene = read_scene_data(root, sequence_set, seq_length, step, img_exts)
        self.img_files, self.poses, self.sample_indices = scene

    def generator(self):
        from PIL import Image

        def load(name):
            return np.asarray(Image.open(name).convert("RGB"), dtype=np.float32)

        for files, gt, windows in zip(self.img_files, self.poses, self.sample_indices):
            for window in windows:
                snippet = gt[np.asarray(window)]                      # [L, 3, 4], a copy
                origin_rot, origin_pos = snippet[0, :, :3].copy(), snippet[0, :, 3].copy()
                snippet[:, :, 3] = snippet[:, :, 3] - origin_pos
                yield dict(imgs=[load(files[i]) for i in window], path=files[0],
                           poses=np.matmul(np.linalg.inv(origin_rot), snippet))

    def __iter__(self):
        return self.generator()

    def __len__(self):
        return int(sum(len(w) for w in self.sample_indices))


def read_scene_data(data_root, sequence_set, seq_length=3, step=1, img_exts=("png",)):
    """<data_root>/sequences/<seq>/image_2/* and <data_root>/poses/<seq>.txt for every directory under sequences/ that
    matches a pattern of ``sequence_set`` -> (image lists, poses [n, 3, 4] float64, snippet indices [N, 2 half + 1]) per
    sequence, in sorted order.  Snippet j is centred on frame j + half step, half = (seq_length - 1) // 2."""
    half = (seq_length - 1) // 2
    offsets = step * np.arange(-half, half + 1)
    found = sorted({d for pattern in sequence_set for d in glob.glob(os.path.join(data_root, "sequences", pattern))
                    if os.path.isdir(d)})
    print("sequences to test: {}".format([os.path.basename(os.path.normpath(d)) for d in found]))
    files, poses, indices = [], [], []
    for directory in found:
        name = os.path.basename(os.path.normpath(directory))
        gt = np.loadtxt(os.path.join(data_root, "poses", name + ".txt"), dtype=np.float64, ndmin=2)
        images = sorted(f for ext in img_exts for f in glob.glob(os.path.join(directory, "image_2", "*." + ext)))
        centres = np.arange(half * step, len(images) - half * step)
        files.append(images)
        poses.append(gt[:, -12:].reshape(-1, 3, 4))
        indices.append(centres[:, None] + offsets[None, :])
    return files, poses, indices
