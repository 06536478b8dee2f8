"""data/prepare_train_data.py end to end on the miniature KITTI-raw tree of the fixtures, the two wrappers replaced by
the host simulator (tests/_prepare_data_cli.py): the dumped tree, its text formats, the removal of short scenes,
--no-train-gt, a split that does not depend on the hash seed, the missing-list error, and the datasets that read it."""
import io
import os
import re
import subprocess
import sys

import numpy as np
import pytest
from PIL import Image

import _prepare_data_cli as C
import _prepare_data_tree as T
from _prepare_data_check import judge_depth, pil_resize

S02, S03 = T.DRIVE + "_02", T.DRIVE + "_03"
V02, V03 = T.DATE + "_drive_0005_sync_02", T.DATE + "_drive_0005_sync_03"
SIZE = ["--height", str(T.HEIGHT), "--width", str(T.WIDTH), "--test-scenes", T.TEST_SCENES]


@pytest.fixture(scope="module")
def raw(tmp_path_factory):
    return T.fixture_tree(str(tmp_path_factory.mktemp("raw")), second_drive=True)


@pytest.fixture(scope="module")
def dump(raw, tmp_path_factory):
    out = str(tmp_path_factory.mktemp("dump"))
    C.run([raw, "--dump-root", out, "--with-depth", "--with-pose", "--num-threads", "2", *SIZE])
    return out


def lines(path):
    return open(path).read().split("\n")[:-1]


def test_layout(dump):
    z = np.load(T.NPZ)
    assert sorted(os.listdir(dump)) == sorted([S02, S03, V02, V03, "train.txt", "val.txt"])  # no test drive
    # the second of the sorted prefixes draws below 0.1 with seed 8964
    assert lines(os.path.join(dump, "train.txt")) == [S02, S03] and lines(os.path.join(dump, "val.txt")) == [V02, V03]
    for scene in (S02, S03, V02, V03):
        want = sorted(["cam.txt", "poses.txt"] + [i + e for i in z["ids"] for e in (".jpg", ".npy")])
        assert sorted(os.listdir(os.path.join(dump, scene))) == want


def test_text_formats(dump):
    z = np.load(T.NPZ)
    number = r"-?\d\.\d{18}e[+-]\d{2}"
    for c, scene in enumerate((S02, S03)):
        cam = lines(os.path.join(dump, scene, "cam.txt"))
        assert len(cam) == 3 and all(re.fullmatch(" ".join([number] * 3), ln) for ln in cam)  # np.savetxt's default
        assert np.allclose(np.genfromtxt(os.path.join(dump, scene, "cam.txt")), z["intrinsics"][c], rtol=1e-12, atol=0)
        poses = lines(os.path.join(dump, scene, "poses.txt"))
        assert len(poses) == 4 and all(re.fullmatch(" ".join([r"-?\d\.\d{6}e[+-]\d{2}"] * 12), ln) for ln in poses)
        buf = io.StringIO()
        np.savetxt(buf, z["poses"][c].reshape(-1, 12), fmt="%.6e")
        got, want = np.genfromtxt(os.path.join(dump, scene, "poses.txt")), np.genfromtxt(io.StringIO(buf.getvalue()))
        # (the goldens' poses in the same format; a last printed digit may differ where 1e-9 of rounding meets a tie)
        assert np.abs(got - want).max() <= 1e-6 * np.maximum(1.0, np.abs(want)).max()


def test_frames_and_depth(dump, tmp_path):
    z = np.load(T.NPZ)
    for c, scene in enumerate((S02, S03)):
        raw_frames = z["frames"] if c == 0 else z["frames"][:, :, ::-1]
        for k, fid in enumerate(z["ids"]):
            small = pil_resize(raw_frames[int(fid)][None], T.HEIGHT, T.WIDTH)[0]
            assert np.array_equal(small, z["imgs"][c][k])  # PIL's resize is what the reference stored
            Image.fromarray(small).save(tmp_path / "want.jpg")
            assert open(os.path.join(dump, scene, fid + ".jpg"), "rb").read() == open(tmp_path / "want.jpg", "rb").read()
        got = np.stack([np.load(os.path.join(dump, scene, fid + ".npy")) for fid in z["ids"]])
        judge_depth(got, z["depth_r1"][c], f"cli on the simulator, {scene}")


def test_depth_size_ratio(raw, tmp_path):
    z = np.load(T.NPZ)
    C.run([raw, "--dump-root", str(tmp_path), "--with-depth", "--depth-size-ratio", "2", "--num-threads", "1", *SIZE])
    got = np.stack([np.load(os.path.join(tmp_path, S03, fid + ".npy")) for fid in z["ids"]])
    judge_depth(got, z["depth_r2"][1], "cli on the simulator, ratio 2")
    assert not os.path.exists(os.path.join(tmp_path, S03, "poses.txt"))
    with pytest.raises(ValueError):
        C.run([raw, "--dump-root", str(tmp_path), "--with-depth", "--depth-size-ratio", "5", *SIZE])


def test_short_scenes_are_removed_and_no_train_gt(raw, tmp_path):
    static = tmp_path / "static.txt"
    with open(static, "w") as f:  # drive 0001 keeps two frames, drive 0005 keeps all eight
        for k in range(6):
            f.write("{} {} {:010d}\n".format(T.DATE, T.DRIVE, k))
    out = str(tmp_path / "dump")
    C.run([raw, "--dump-root", out, "--static-frames", str(static), "--with-depth", "--no-train-gt", *SIZE])
    assert sorted(os.listdir(out)) == sorted([V02, V03, "train.txt", "val.txt"])
    # one prefix is left: the first draw sends it to train, and its depth maps are deleted
    assert lines(os.path.join(out, "train.txt")) == [V02, V03] and lines(os.path.join(out, "val.txt")) == []
    names = os.listdir(os.path.join(out, V02))
    assert sum(n.endswith(".jpg") for n in names) == 8 and not any(n.endswith(".npy") for n in names)


def test_no_train_gt_keeps_the_validation_depth(raw, tmp_path):
    C.run([raw, "--dump-root", str(tmp_path), "--with-depth", "--no-train-gt", *SIZE])
    assert not any(n.endswith(".npy") for n in os.listdir(tmp_path / S02))
    assert sum(n.endswith(".npy") for n in os.listdir(tmp_path / V02)) == 4


def test_split_does_not_depend_on_the_hash_seed(raw, dump, tmp_path):
    for seed in ("1", "2"):
        out = str(tmp_path / seed)
        env = dict(os.environ, PYTHONHASHSEED=seed)
        res = subprocess.run([sys.executable, C.__file__, raw, "--dump-root", out, *SIZE], env=env, capture_output=True,
                             text=True, timeout=300)
        assert res.returncode == 0, res.stderr[-3000:]
        for name in ("train.txt", "val.txt"):
            assert open(os.path.join(out, name)).read() == open(os.path.join(dump, name)).read()


def test_missing_list_of_test_scenes(raw, tmp_path):
    missing = str(tmp_path / "nowhere.txt")
    with pytest.raises(SystemExit) as e:
        C.run([raw, "--dump-root", str(tmp_path / "d"), "--height", "16", "--width", "48", "--test-scenes", missing])
    assert missing in str(e.value) and "--test-scenes" in str(e.value)
    assert not os.path.isfile(C.cli.DEFAULT_TEST_SCENES)  # the product ships no list ...
    with pytest.raises(SystemExit) as e:                    # ... and says which file it looks for
        C.run([raw, "--dump-root", str(tmp_path / "d"), "--height", "16", "--width", "48"])
    assert C.cli.DEFAULT_TEST_SCENES in str(e.value)
    assert not os.path.exists(tmp_path / "d" / "train.txt")


def test_flags_are_the_reference_s():
    opts = {a.dest: a for a in C.cli.parser._actions}
    assert opts["dataset_format"].choices == ["kitti_raw", "cityscapes", "kitti_odom"] and opts["dataset_format"].default == "kitti_raw"
    assert (opts["height"].default, opts["width"].default, opts["depth_size_ratio"].default, opts["num_threads"].default,
            opts["dump_root"].default, opts["static_frames"].default) == (128, 416, 1, 4, "dump", None)
    assert {"with_depth", "with_pose", "no_train_gt", "test_scenes", "dataset_dir"} <= set(opts)


def test_the_prepared_tree_loads(dump):
    from datasets.sequence_folders import SequenceFolder
    from datasets.validation_folders import ValidationSet
    train = SequenceFolder(dump, seed=0, train=True, sequence_length=3)
    assert len(train) == 4  # two cameras, four frames each: two triplets per camera
    tgt, refs, K, K_inv = train[0]
    assert tgt.shape == (T.HEIGHT, T.WIDTH, 3) and len(refs) == 2 and K.shape == (3, 3) and np.isfinite(K_inv).all()
    val = ValidationSet(dump, dataset="kitti")
    assert len(val) == 8
    img, depth = val[0]
    assert img.shape == (T.HEIGHT, T.WIDTH, 3) and tuple(depth.shape) == (T.HEIGHT, T.WIDTH) and (depth > 0).any()


def test_other_formats_run(tmp_path_factory):
    odom = T.write_kitti_odom(str(tmp_path_factory.mktemp("odom")))
    out = str(tmp_path_factory.mktemp("odomdump"))
    C.run([odom, "--dataset-format", "kitti_odom", "--dump-root", out, "--height", "10", "--width", "32"])
    assert sorted(d for d in os.listdir(out) if not d.endswith(".txt")) == ["00_2", "00_3", "03_2", "03_3"]
    assert Image.open(os.path.join(out, "00_2", "000000.jpg")).size == (32, 10)
    city = T.write_cityscapes(str(tmp_path_factory.mktemp("cs")))
    out = str(tmp_path_factory.mktemp("csdump"))
    C.run([city, "--dataset-format", "cityscapes", "--dump-root", out, "--height", "16", "--width", "32"])
    scenes = [d for d in os.listdir(out) if not d.endswith(".txt")]
    assert scenes and all(len([f for f in os.listdir(os.path.join(out, d)) if f.endswith(".jpg")]) >= 3 for d in scenes)
    first = os.path.join(out, scenes[0])
    jpg = sorted(f for f in os.listdir(first) if f.endswith(".jpg"))[0]
    assert Image.open(os.path.join(first, jpg)).size == (32, 12)  # the bottom quarter is not kept
