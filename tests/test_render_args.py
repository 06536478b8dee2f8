"""reconstruct.py's handling of the render flags, where no device is needed: --render-poses' file is read and checked
before anything else, and --render and --render-poses without a HIP device end as the program always ends without one."""
import numpy as np
import pytest
import torch

import reconstruct

BASE = ["--pretrained-dispnet", "none.pth.tar", "--pretrained-posenet", "none.pth.tar", "--dataset-dir", "none",
        "--intrinsics", "none.txt"]


def test_flags_and_defaults():
    args = reconstruct.parser.parse_args(BASE)
    assert args.render is False and args.render_poses is None and args.render_step is None and args.render_near == 0.0
    args = reconstruct.parser.parse_args(BASE + ["--render", "--render-poses", "p.txt", "--render-step", "0.02",
                                                 "--render-near", "0.3"])
    assert args.render is True and args.render_poses == "p.txt" and args.render_step == 0.02 and args.render_near == 0.3


def test_read_poses_takes_poses_txt(tmp_path):
    poses = np.random.default_rng(1).standard_normal((4, 12))
    path = tmp_path / "poses.txt"
    np.savetxt(str(path), poses, delimiter=' ', fmt='%1.8e')
    got = reconstruct.read_poses(str(path))
    want = np.array([[float("%1.8e" % v) for v in row] for row in poses]).reshape(4, 3, 4)
    assert got.dtype == np.float64 and got.shape == (4, 3, 4) and np.array_equal(got, want)


@pytest.mark.parametrize("text", ["", "1 2 3\n", "1 0 0 0 0 1 0 0 0 0 1\n", "1 0 0 0 0 1 0 0 0 0 1 0 7\n",
                                  "1 0 0 0 0 1 0 0 0 0 1 x\n", "1 0 0 0 0 1 0 0 0 0 1 nan\n",
                                  "1 0 0 0 0 1 0 0 0 0 1 0\n1 0 0 inf 0 1 0 0 0 0 1 0\n"])
def test_a_malformed_pose_file_is_refused_by_the_flags_name(tmp_path, text):
    path = tmp_path / "bad.txt"
    path.write_text(text)
    with pytest.raises(SystemExit, match="--render-poses"):
        reconstruct.main(BASE + ["--render-poses", str(path)])
    with pytest.raises(SystemExit, match="--render-poses"):
        reconstruct.read_poses(str(path))


def test_a_missing_pose_file_is_refused(tmp_path):
    with pytest.raises(SystemExit, match="--render-poses"):
        reconstruct.main(BASE + ["--render-poses", str(tmp_path / "none.txt")])


def test_bad_march_flags_are_refused():
    for flags, name in ((["--render-step", "0"], "--render-step"), (["--render-step", "nan"], "--render-step"),
                        (["--render-near", "-1"], "--render-near")):
        with pytest.raises(SystemExit, match=name):
            reconstruct.main(BASE + ["--render"] + flags)


def test_both_flags_without_a_device(tmp_path, monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    path = tmp_path / "poses.txt"
    np.savetxt(str(path), np.eye(4)[:3].reshape(1, 12), fmt='%1.8e')
    for flags in (["--render"], ["--render-poses", str(path)], ["--render", "--render-poses", str(path)]):
        with pytest.raises(SystemExit, match="needs a HIP device"):
            reconstruct.main(BASE + flags)
