"""Runs the reference's own compute_pose_error (test_pose.py) and test_framework_KITTI.generator
(kitti_eval/pose_evaluation_utils.py).  The two modules are imported with skimage, path, imageio and tqdm replaced by
empty stand-ins for the duration of the import (none of them is installed here, and none takes part in the arithmetic);
the framework object is made with __new__ and given its file names, poses and snippet indices by hand, because
read_scene_data needs ``path``; the stand-in imread returns a black pixel."""
from __future__ import annotations

import importlib.util
import os
import sys
import types

import numpy as np

REFERENCE = os.environ.get("SCSFM_REFERENCE", "/root/reference")
TEST_POSE = os.path.join(REFERENCE, "test_pose.py")
UTILS = os.path.join(REFERENCE, "kitti_eval", "pose_evaluation_utils.py")
STUBBED = ("skimage", "skimage.transform", "path", "imageio", "tqdm")


def available():
    return os.path.isfile(TEST_POSE) and os.path.isfile(UTILS)


def _stand_ins():
    mods = {k: types.ModuleType(k) for k in STUBBED}
    mods["skimage"].transform = mods["skimage.transform"]
    mods["skimage.transform"].resize = lambda img, shape, *a, **k: img
    mods["path"].Path = str
    mods["imageio"].imread = lambda name: np.zeros((1, 1, 3), np.uint8)
    mods["tqdm"].tqdm = lambda it, *a, **k: it
    return mods


def _load(name, path):
    saved = {k: sys.modules.get(k) for k in STUBBED}
    sys.modules.update(_stand_ins())
    try:
        spec = importlib.util.spec_from_file_location(name, path)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    return mod


_cache = {}


def modules():
    if not _cache:
        _cache["test_pose"] = _load("_reference_test_pose", TEST_POSE)
        _cache["utils"] = _load("_reference_pose_evaluation_utils", UTILS)
    return _cache["test_pose"], _cache["utils"]


def compensated(gts, L=5):
    """gts: a list of [n, 12] / [n, 3, 4] arrays -> [N, L, 3, 4]: what the reference's generator yields as 'poses', for
    every snippet of every sequence in order."""
    _, utils = modules()
    fw = utils.test_framework_KITTI.__new__(utils.test_framework_KITTI)
    fw.root = ""
    fw.poses = [np.asarray(g, np.float64).reshape(-1, 3, 4) for g in gts]
    fw.img_files = [["{:06d}.png".format(i) for i in range(len(p))] for p in fw.poses]
    fw.sample_indices = [np.arange(max(len(p) - L + 1, 0))[:, None] + np.arange(L)[None] for p in fw.poses]
    out = [sample["poses"] for sample in fw]
    return np.array(out, np.float64).reshape(-1, L, 3, 4)


def pose_errors(gt_comp, pred):
    """compute_pose_error snippet by snippet -> float64 [N, 2]."""
    test_pose, _ = modules()
    return np.array([[float(x) for x in test_pose.compute_pose_error(g, p)] for g, p in zip(gt_comp, pred)],
                    np.float64).reshape(-1, 2)


def stats(errors):
    """mean and std as the reference's main() takes them: of a float32 array -> two float32 [2]."""
    e = np.zeros((len(errors), 2), np.float32)
    for j, (ate, re) in enumerate(errors):
        e[j] = ate, re
    return e.mean(0), e.std(0)
