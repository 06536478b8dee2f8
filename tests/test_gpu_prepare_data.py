"""data/prepare_train_data.py end to end on the GPU, on the miniature KITTI-raw tree of the fixtures: the frames PIL's own
bytes, the depth maps, intrinsics and poses the goldens', and a tree that train.py trains on."""
import os
import subprocess
import sys

import numpy as np
import pytest
from PIL import Image

import _prepare_data_tree as T
from _prepare_data_check import judge_depth, pil_resize

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "sc-sfmlearner-release_amd")
CLI = os.path.join(PKG, "data", "prepare_train_data.py")


def prepare(raw, out, *extra):
    res = subprocess.run([sys.executable, CLI, raw, "--dump-root", out, "--test-scenes", T.TEST_SCENES, *extra],
                         env=dict(os.environ, PYTHONPATH=PKG), capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]


@pytest.fixture(scope="module")
def raw(tmp_path_factory):
    return T.fixture_tree(str(tmp_path_factory.mktemp("raw")), second_drive=True)


def test_cli_on_the_fixture_drive(raw, tmp_path):
    z = np.load(T.NPZ)
    out = str(tmp_path / "dump")
    prepare(raw, out, "--with-depth", "--with-pose", "--num-threads", "2", "--height", str(T.HEIGHT), "--width", str(T.WIDTH))
    for c, cid in enumerate(("02", "03")):
        scene = os.path.join(out, T.DRIVE + "_" + cid)
        raw_frames = z["frames"] if c == 0 else z["frames"][:, :, ::-1]
        for fid in z["ids"]:
            Image.fromarray(pil_resize(raw_frames[int(fid)][None], T.HEIGHT, T.WIDTH)[0]).save(tmp_path / "want.jpg")
            assert open(os.path.join(scene, fid + ".jpg"), "rb").read() == open(tmp_path / "want.jpg", "rb").read()
        got = np.stack([np.load(os.path.join(scene, fid + ".npy")) for fid in z["ids"]])
        judge_depth(got, z["depth_r1"][c], f"cli on the gpu, camera {cid}")
        assert np.allclose(np.genfromtxt(os.path.join(scene, "cam.txt")), z["intrinsics"][c], rtol=1e-12, atol=0)
        poses = np.genfromtxt(os.path.join(scene, "poses.txt")).reshape(-1, 3, 4)
        want = z["poses"][c]
        # six printed decimals of the mantissa, then the issue's bounds: 1e-9 (rotation), 1e-6 m (translation)
        assert np.abs(poses - want).max() <= 5.1e-7 * np.maximum(1.0, np.abs(want)).max() + 1e-6
    assert open(os.path.join(out, "val.txt")).read().split() == [T.DATE + "_drive_0005_sync_02", T.DATE + "_drive_0005_sync_03"]


def test_train_py_takes_three_steps_on_a_prepared_tree(raw, tmp_path):
    static = tmp_path / "static.txt"
    static.write_text("{} {}_drive_0009_sync 0000000000\n".format(T.DATE, T.DATE))  # names no frame here: all 8 are kept
    out = str(tmp_path / "dump")
    prepare(raw, out, "--static-frames", str(static), "--height", "128", "--width", "416")
    cmd = [sys.executable, os.path.join(PKG, "train.py"), out, "--resnet-layers", "18", "-b", "2", "--epoch-size", "3",
           "--epochs", "1", "--with-pretrain", "0", "-j", "0", "--name", "prepared"]
    env = dict(os.environ, PYTHONPATH=PKG, SCSFM_CUDNN_BENCHMARK="0")
    res = subprocess.run(cmd, cwd=tmp_path, env=env, capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    run_dir = os.path.join(tmp_path, "checkpoints", "prepared")
    stamp = os.listdir(run_dir)[0]
    rows = open(os.path.join(run_dir, stamp, "progress_log_full.csv")).read().strip().split("\n")
    vals = [[float(v) for v in r.split("\t")] for r in rows[1:]]
    assert len(vals) == 3 and all(np.isfinite(v) and abs(v) < 1e3 for r in vals for v in r)
