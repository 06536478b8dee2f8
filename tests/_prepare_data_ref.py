"""Runs the reference's own loaders (data/kitti_raw_loader.py, data/kitti_odom_loader.py, data/cityscapes_loader.py) on
a current stack.  They are imported with ``path`` replaced by a small str subclass that has the handful of methods
the loaders use, ``scipy.misc`` by PIL (imread = open -> array, imresize = Image.resize((w, h), BILINEAR), which is
what scipy.misc.imresize was) and ``tqdm`` by a pass-through; ``np.int`` is given back for the duration of a call and
removed afterwards."""
from __future__ import annotations

import contextlib
import fnmatch
import importlib.util
import os
import sys
import types

import numpy as np
from PIL import Image

REFERENCE = os.environ.get("SCSFM_REFERENCE", "/root/reference")
DATA = os.path.join(REFERENCE, "data")
STUBBED = ("path", "scipy", "scipy.misc", "tqdm")


def available():
    return all(os.path.isfile(os.path.join(DATA, f)) for f in
               ("kitti_raw_loader.py", "kitti_odom_loader.py", "cityscapes_loader.py", "test_scenes.txt"))


class Path(str):
    def __truediv__(self, other):
        return Path(os.path.join(self, other))

    def __add__(self, other):
        return Path(str(self) + other)

    name = property(lambda self: os.path.basename(self))
    parent = property(lambda self: Path(os.path.dirname(self)))

    def basename(self):
        return Path(os.path.basename(self))

    def dirname(self):
        return Path(os.path.dirname(self))

    def realpath(self):
        return Path(os.path.realpath(self))

    def isfile(self):
        return os.path.isfile(self)

    def _list(self, pattern, test):
        return [Path(os.path.join(self, f)) for f in os.listdir(self)
                if test(os.path.join(self, f)) and (pattern is None or fnmatch.fnmatch(f, pattern))]

    def dirs(self, pattern=None):
        return self._list(pattern, os.path.isdir)

    def files(self, pattern=None):
        return self._list(pattern, os.path.isfile)


def _stand_ins():
    mods = {k: types.ModuleType(k) for k in STUBBED}
    mods["path"].Path = Path
    mods["scipy"].misc = mods["scipy.misc"]
    mods["scipy.misc"].imread = lambda f: np.array(Image.open(f))
    mods["scipy.misc"].imresize = lambda img, size: np.array(Image.fromarray(img).resize((size[1], size[0]), Image.BILINEAR))
    mods["tqdm"].tqdm = lambda it, *a, **k: it
    return mods


def _load(name):
    saved = {k: sys.modules.get(k) for k in STUBBED}
    sys.modules.update(_stand_ins())
    try:
        spec = importlib.util.spec_from_file_location("_reference_" + name, os.path.join(DATA, name + ".py"))
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


def module(name):
    if name not in _cache:
        _cache[name] = _load(name)
    return _cache[name]


@contextlib.contextmanager
def old_numpy():
    had = "int" in np.__dict__
    if not had:
        np.int = int
    try:
        yield
    finally:
        if not had:
            del np.int


def _describe(loader, frames=True):
    """Every scene of the loader -> list of dict(rel_path, intrinsics, ids, [poses, depths, imgs])."""
    out = []
    with old_numpy():
        for drive in sorted(loader.scenes):
            for scene in loader.collect_scenes(drive):
                rec = {"rel_path": str(scene["rel_path"]), "intrinsics": np.array(scene["intrinsics"])}
                samples = list(loader.get_scene_imgs(scene)) if frames else []
                rec["ids"] = [str(s["id"]) for s in samples]
                rec["imgs"] = [s["img"] for s in samples]
                if samples and "pose" in samples[0]:
                    rec["poses"] = np.array([s["pose"] for s in samples])
                if samples and "depth" in samples[0]:
                    rec["depths"] = np.array([s["depth"] for s in samples])
                out.append(rec)
    return out


def kitti_raw(root, height, width, static_frames_file=None, get_depth=False, get_pose=False, depth_size_ratio=1):
    mod = module("kitti_raw_loader")
    with old_numpy():
        loader = mod.KittiRawLoader(root, static_frames_file=static_frames_file, img_height=height, img_width=width,
                                    get_depth=get_depth, get_pose=get_pose, depth_size_ratio=depth_size_ratio)
    return _describe(loader)


def kitti_odom(root, height, width):
    return _describe(module("kitti_odom_loader").KittiOdomLoader(root, img_height=height, img_width=width))


def cityscapes(root, height, width):
    """(Sub-sequences without frames are described without asking for their images: the reference's generator prints
    the first frame id of a scene before it looks at it, which fails on an empty one.)"""
    loader = module("cityscapes_loader").cityscapes_loader(root, img_height=height, img_width=width)
    out = []
    for city in sorted(loader.scenes):
        for scene in loader.collect_scenes(city):
            rec = {"rel_path": str(scene["rel_path"]), "intrinsics": np.array(scene["intrinsics"])}
            samples = list(loader.get_scene_imgs(scene)) if scene["frame_ids"] else []
            rec["ids"] = [str(s["id"]) for s in samples]
            rec["imgs"] = [s["img"] for s in samples]
            out.append(rec)
    return out


def depth_map(P_rect, scan_file, calib_dir, height, width, ratio):
    """generate_depth_map for one scan file, on a loader object made by hand."""
    mod = module("kitti_raw_loader")
    loader = mod.KittiRawLoader.__new__(mod.KittiRawLoader)
    loader.img_height, loader.img_width, loader.depth_size_ratio = height, width, ratio
    d = Path(os.path.dirname(os.path.dirname(os.path.dirname(scan_file))))
    assert os.path.samefile(d.parent, calib_dir)
    scene = {"dir": d, "P_rect": np.array(P_rect), "frame_id": [os.path.basename(scan_file)[:-4]]}
    with old_numpy():
        return loader.generate_depth_map(scene, 0)
