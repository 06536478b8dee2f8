"""Prepare a raw KITTI / KITTI odometry / Cityscapes download for train.py: one folder per scene and camera with cam.txt,
poses.txt, <frame>.jpg and <frame>.npy, plus train.txt and val.txt.

    python data/prepare_train_data.py /data/kitti_raw --dataset-format kitti_raw --dump-root /data/kitti_256 \
        --width 832 --height 256 --with-depth --with-pose --test-scenes data/test_scenes.txt

The frames are resized and the Velodyne scans projected on the GPU (scsfm_hip.prepare: libscsfm_prep.so).  One process
opens the GPU; --num-threads host threads decode the PNGs and encode the JPEGs.
"""
from __future__ import annotations

import argparse
import os
import shutil
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (HERE, os.path.dirname(HERE)):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np  # noqa: E402
import torch  # noqa: E402
from PIL import Image  # noqa: E402

from scsfm_hip import prepare as hip_prepare  # noqa: E402

MAX_THREADS = 16
BATCH = 32  # frames staged, resized and copied back together
DEFAULT_TEST_SCENES = os.path.join(HERE, "test_scenes.txt")

parser = argparse.ArgumentParser()
parser.add_argument("dataset_dir", metavar='DIR',
                    help='path to original dataset')
parser.add_argument("--dataset-format", type=str, default='kitti_raw', choices=["kitti_raw", "cityscapes", "kitti_odom"])
parser.add_argument("--static-frames", default=None,
                    help="list of imgs to discard for being static, if not set will discard them based on speed \
                    (careful, on KITTI some frames have incorrect speed)")
parser.add_argument("--with-depth", action='store_true',
                    help="If available (e.g. with KITTI), will store depth ground truth along with images, for validation")
parser.add_argument("--with-pose", action='store_true',
                    help="If available (e.g. with KITTI), will store pose ground truth along with images, for validation")
parser.add_argument("--no-train-gt", action='store_true',
                    help="If selected, will delete ground truth depth to save space")
parser.add_argument("--dump-root", type=str, default='dump', help="Where to dump the data")
parser.add_argument("--height", type=int, default=128, help="image height")
parser.add_argument("--width", type=int, default=416, help="image width")
parser.add_argument("--depth-size-ratio", type=int, default=1, help="will divide depth size by that ratio")
parser.add_argument("--num-threads", type=int, default=4, help="number of threads to use")
parser.add_argument("--test-scenes", default=None,
                    help="kitti_raw: list of the drives kept for testing, one per line (default: test_scenes.txt next "
                         "to this script)")


def read_test_scenes(path):
    """The drives to leave out, one per line.  Without a list kitti_raw is not prepared at all: the test drives would
    end up in the training set."""
    path = path or DEFAULT_TEST_SCENES
    if not os.path.isfile(path):
        raise SystemExit(f"prepare_train_data.py: kitti_raw needs the list of test scenes, {path} does not exist "
                         "(name one with --test-scenes)")
    with open(path) as f:
        return [line.strip() for line in f if line.strip()]


def make_loader(args):
    if args.dataset_format == 'kitti_raw':
        from kitti_raw_loader import KittiRawLoader
        return KittiRawLoader(args.dataset_dir, read_test_scenes(args.test_scenes),
                              static_frames_file=args.static_frames, img_height=args.height, img_width=args.width,
                              get_depth=args.with_depth, get_pose=args.with_pose,
                              depth_size_ratio=args.depth_size_ratio)
    if args.dataset_format == 'kitti_odom':
        from kitti_odom_loader import KittiOdomLoader
        return KittiOdomLoader(args.dataset_dir, img_height=args.height, img_width=args.width)
    from cityscapes_loader import cityscapes_loader
    return cityscapes_loader(args.dataset_dir, img_height=args.height, img_width=args.width)


def decode(path):
    """A PNG as uint8 [H, W, C]."""
    with Image.open(path) as im:
        a = np.asarray(im)
    if a.dtype != np.uint8:
        raise ValueError(f"{path}: only 8-bit images can be prepared, got {a.dtype}")
    return a[:, :, None] if a.ndim == 2 else a


def encode(path, img):
    """PIL's JPEG with its defaults."""
    Image.fromarray(img[:, :, 0] if img.shape[2] == 1 else img).save(path)


def dump_frames(loader, scene, frames, dump_dir, device, pool):
    """One batch: decode on the pool, one resize call per frame size, one copy back, encode on the pool; with depth,
    the batch's scans through one velodyne_depth call."""
    images = list(pool.map(decode, [fr["img_file"] for fr in frames]))
    by_shape = {}
    for k, a in enumerate(images):
        by_shape.setdefault(a.shape, []).append(k)
    small = [None] * len(frames)
    for idx in by_shape.values():
        staged = torch.from_numpy(np.stack([images[k] for k in idx])).to(device)
        out = hip_prepare.resize_u8(staged, loader.img_height, loader.img_width, loader.keep_rows).cpu().numpy()
        for k, img in zip(idx, out):
            small[k] = img
    list(pool.map(encode, [os.path.join(dump_dir, fr["id"] + ".jpg") for fr in frames], small))
    if "velo_file" in frames[0]:
        scans = list(pool.map(lambda f: np.fromfile(f, dtype=np.float32).reshape(-1, 4), [fr["velo_file"] for fr in frames]))
        off = np.concatenate([[0], np.cumsum([len(s) for s in scans])]).astype(np.int32)
        h, w, bounds = loader.depth_size
        P = np.repeat(scene["P_velo2im"][None], len(scans), axis=0)
        depth = hip_prepare.velodyne_depth(torch.from_numpy(np.concatenate(scans)).to(device),
                                           torch.from_numpy(off).to(device), torch.from_numpy(P).to(device), h, w,
                                           bounds).cpu().numpy()
        for fr, d in zip(frames, depth):
            np.save(os.path.join(dump_dir, fr["id"] + ".npy"), d)


def dump_example(args, loader, drive, device, pool):
    for scene in loader.collect_scenes(drive):
        dump_dir = os.path.join(args.dump_root, scene["rel_path"])
        os.makedirs(dump_dir, exist_ok=True)
        np.savetxt(os.path.join(dump_dir, "cam.txt"), scene["intrinsics"])
        frames = loader.frames(scene)
        for start in range(0, len(frames), BATCH):
            dump_frames(loader, scene, frames[start:start + BATCH], dump_dir, device, pool)
        poses = [fr["pose"].tolist() for fr in frames if "pose" in fr]
        if poses:
            np.savetxt(os.path.join(dump_dir, "poses.txt"), np.array(poses).reshape(-1, 12), fmt='%.6e')
        if len([f for f in os.listdir(dump_dir) if f.endswith(".jpg")]) < 3:
            shutil.rmtree(dump_dir)


def write_split(args):
    """train.txt / val.txt: the two cameras of a scene fall into the same set.  The prefixes are sorted before the
    draws, so the split does not depend on the interpreter's hash seed."""
    np.random.seed(8964)
    subdirs = sorted(d for d in os.listdir(args.dump_root) if os.path.isdir(os.path.join(args.dump_root, d)))
    prefixes = sorted({d[:-2] for d in subdirs})
    with open(os.path.join(args.dump_root, "train.txt"), "w") as tf, open(os.path.join(args.dump_root, "val.txt"), "w") as vf:
        for pr in prefixes:
            members = [d for d in subdirs if d.startswith(pr)]
            if np.random.random() < 0.1:
                for d in members:
                    vf.write("{}\n".format(d))
            else:
                for d in members:
                    tf.write("{}\n".format(d))
                    if args.with_depth and args.no_train_gt:
                        for f in os.listdir(os.path.join(args.dump_root, d)):
                            if f.endswith(".npy"):
                                os.remove(os.path.join(args.dump_root, d, f))


def run(args, device):
    os.makedirs(args.dump_root, exist_ok=True)
    loader = make_loader(args)
    print('Found {} potential scenes'.format(len(loader.scenes)))
    print('Retrieving frames')
    with ThreadPoolExecutor(max_workers=max(1, min(args.num_threads, MAX_THREADS))) as pool:
        for drive in loader.scenes:
            dump_example(args, loader, drive, device, pool)
    print('Generating train val lists')
    write_split(args)


def main(argv=None):
    args = parser.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("prepare_train_data.py needs a HIP device")
    run(args, torch.device("cuda"))


if __name__ == '__main__':
    main()
