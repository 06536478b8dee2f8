"""reconstruct.py's handling of --follow, where no device is needed: the flags, their defaults and the docstring; what is
refused at the top of main, before the device check; and the policy that places the window (scsfm_hip.rolling.shift_for,
initial_origin, keep_box, origin_at) against values worked out by hand."""
import numpy as np
import pytest
import torch

import reconstruct
import rolling_oracle as RO
from scsfm_hip import rolling

BASE = ["--pretrained-dispnet", "none.pth.tar", "--pretrained-posenet", "none.pth.tar", "--dataset-dir", "none",
        "--intrinsics", "none.txt"]


def test_flags_and_defaults():
    args = reconstruct.parser.parse_args(BASE)
    assert args.follow is False and args.follow_dims is None and args.follow_step is None     # (filled in by main)
    args = reconstruct.parser.parse_args(BASE + ["--follow", "--follow-dims", "64", "32", "48", "--follow-step", "4"])
    assert args.follow and args.follow_dims == [64, 32, 48] and args.follow_step == 4
    with pytest.raises(SystemExit):
        reconstruct.parser.parse_args(BASE + ["--follow", "--follow-dims", "64", "32"])
    for word in ("--follow", "--follow-dims", "--follow-step", "scsfm_hip.rolling", "libscsfm_roll.so", "96 bytes",
                 "len // 2", "--mesh, --render and --render-poses are refused", "Without --follow every file and printed"):
        assert word in reconstruct.__doc__, word
    assert "on_shift(shift, offset, xyz, rgb)" in reconstruct.main.__doc__
    assert reconstruct.FOLLOW_STEP == 8


def test_the_default_window():
    """a cube of side 2 (max_depth + trunc) / voxel + 2 step, rounded up to a multiple of 8"""
    def dims(*flags):
        args = reconstruct.parser.parse_args(BASE + ["--follow", *flags])
        reconstruct.follow_arguments(args)
        return args.follow_dims, args.follow_step
    # 2 (10 + 0.15) / 0.05 + 16 = 422 -> 424
    assert dims("--voxel-size", "0.05") == ([424, 424, 424], 8)
    # 2 (1.5 + 0.375) / 0.125 + 16 = 46 -> 48; with a step of 1: 32; with a truncation of 0.5: 2 x 2 / 0.125 + 16 = 48
    assert dims("--voxel-size", "0.125", "--max-depth", "1.5") == ([48, 48, 48], 8)
    assert dims("--voxel-size", "0.125", "--max-depth", "1.5", "--follow-step", "1") == ([32, 32, 32], 1)
    assert dims("--voxel-size", "0.125", "--max-depth", "1.5", "--trunc", "0.5") == ([48, 48, 48], 8)
    assert dims("--voxel-size", "0.125", "--follow-dims", "40", "16", "48") == ([40, 16, 48], 8)
    assert dims("--voxel-size", "1", "--follow-dims", "1024", "1024", "512")[0] == [1024, 1024, 512]      # (2^29 itself)


@pytest.mark.parametrize("flags, words", [
    (["--follow-dims", "8", "8", "8"], "--follow-dims needs --follow"),
    (["--follow-step", "8"], "--follow-step needs --follow"),
    (["--voxel-size", "0.1", "--follow-step", "4"], "--follow-step needs --follow"),
    (["--follow"], "--follow needs --voxel-size"),
    (["--follow", "--resolution", "128"], "--follow needs --voxel-size"),
    (["--follow", "--voxel-size", "0"], "--voxel-size must be positive"),
    (["--follow", "--voxel-size", "0.1", "--mesh"], "--follow cannot be combined with --mesh"),
    (["--follow", "--voxel-size", "0.1", "--render"], "--follow cannot be combined with --render"),
    (["--follow", "--voxel-size", "0.1", "--render-poses", "no_such_file.txt"], "--follow cannot be combined with --render-poses"),
    (["--follow", "--voxel-size", "0.1", "--follow-step", "0"], "--follow-step must be at least 1"),
    (["--follow", "--voxel-size", "0.1", "--follow-step", "-8"], "--follow-step must be at least 1"),
    (["--follow", "--voxel-size", "0.1", "--follow-dims", "0", "8", "8"], "--follow-dims must all be at least 1"),
    (["--follow", "--voxel-size", "0.1", "--follow-dims", "8", "8", "-1"], "--follow-dims must all be at least 1"),
    (["--follow", "--voxel-size", "0.1", "--follow-dims", "1024", "1024", "513"], "above the limit of 2\\^29"),
    (["--follow", "--voxel-size", "0.001", "--max-depth", "10"], "above the limit of 2\\^29"),
])
def test_refused_before_the_device_check(flags, words, monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(SystemExit, match=words):
        reconstruct.main(BASE + flags)


def test_good_values_without_a_device(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    for flags in (["--follow", "--voxel-size", "0.05"], ["--follow", "--voxel-size", "0.05", "--follow-step", "1"],
                  ["--follow", "--voxel-size", "0.05", "--follow-dims", "512", "128", "512", "--consistency-weight",
                   "--refine-poses"], ["--voxel-size", "0.05", "--mesh", "--render"], []):
        with pytest.raises(SystemExit, match="needs a HIP device"):
            reconstruct.main(BASE + flags)


def test_shift_for_against_hand_computed_values():
    dims, o0 = (16, 16, 16), (0.0, 0.0, 0.0)
    # voxel 0.5, window 16: the central cell is 8.  A centre exactly on the boundary of cells 15 and 16 (8.0) is in cell 16:
    # off 8 -> one step; just below it (7.999) cell 15: off 7 = step - 1 -> nothing; 0.25: cell 0, off -8 = -step -> -8
    assert rolling.shift_for((8.0, 7.999, 0.25), o0, (0, 0, 0), dims, 0.5, 8) == (8, 0, -8)
    # off 17 -> 16 (truncated towards zero, not rounded), off -15 -> -8, off -16 -> -16
    assert rolling.shift_for((12.6, -3.4, -4.0), o0, (0, 0, 0), dims, 0.5, 8) == (16, -8, -16)
    # a negative offset: the window starts at voxel -16.  -8.25 / 0.5 = -16.5 -> floor -17, cell -1, off -9 -> -8;
    # -4.0: cell 8 -> 0; 0.1: cell 16, off 8 -> 8
    assert rolling.shift_for((-8.25, -4.0, 0.1), o0, (-16, -16, -16), dims, 0.5, 8) == (-8, 0, 8)
    # step 1: the window follows cell by cell; off 3, -3 and 0
    assert rolling.shift_for((5.6, 2.6, 4.3), o0, (0, 0, 0), dims, 0.5, 1) == (3, -3, 0)
    # per-axis dims, an origin0 off zero, an odd size (the central cell of 5 is 2)
    assert rolling.shift_for((1.0, 1.0, 1.0), (-1.0, 0.5, 1.0), (0, 0, 0), (5, 4, 2), 0.25, 2) == (6, 0, 0) \
        and rolling.shift_for((1.0, 1.0, 1.0), (-1.0, 0.5, 1.0), (0, 0, 0), (5, 4, 2), 0.25, 1) == (6, 0, -1)
    with pytest.raises(ValueError, match="step"):
        rolling.shift_for((0, 0, 0), o0, (0, 0, 0), dims, 0.5, 0)
    # and the oracle's restatement says the same
    rng = np.random.default_rng(5)
    for _ in range(200):
        c, o = rng.uniform(-20, 20, 3), rng.uniform(-5, 5, 3)
        k, n = tuple(int(v) for v in rng.integers(-40, 40, 3)), tuple(int(v) for v in rng.integers(1, 50, 3))
        step = int(rng.integers(1, 10))
        got = rolling.shift_for(c, o, k, n, 0.125, step)
        assert got == RO.shift_for(c, o, k, n, 0.125, step) and all(isinstance(v, int) and v % step == 0 for v in got)


def test_initial_origin_keep_box_and_origin_at():
    got = rolling.initial_origin((1.0, -2.0, 0.25), (40, 16, 47), 0.125)
    assert got == (1.0 - 20.5 * 0.125, -2.0 - 8.5 * 0.125, 0.25 - 23.5 * 0.125) == (-1.5625, -3.0625, -2.6875)
    # the camera it was made for sits in the central cell: nothing moves, with any step
    for step in (1, 8):
        assert rolling.shift_for((1.0, -2.0, 0.25), got, (0, 0, 0), (40, 16, 47), 0.125, step) == (0, 0, 0)
    assert rolling.keep_box((37, 18, 29), (8, 0, 0)) == (8, 37, 0, 18, 0, 29)
    assert rolling.keep_box((37, 18, 29), (-3, 5, -7)) == (0, 34, 5, 18, 0, 22)
    assert rolling.keep_box((37, 18, 29), (0, 18, -40)) == (0, 37, 18, 18, 0, -11)       # (empty on y and on z)
    assert rolling.keep_box((37, 18, 29), (0, 0, 0)) == (0, 37, 0, 18, 0, 29) == RO.keep_box((37, 18, 29), (0, 0, 0))
    # fl(origin0 + fl(float(k) s)) in fp32: recomputed from k, so k steps of one are the same as one step of k
    o = rolling.origin_at((-2.5, 0.1, 3.0), (16, 7, -64), 0.125)
    assert o == (-0.5, float(np.float32(0.1) + np.float32(7) * np.float32(0.125)), -5.0)
    assert o == tuple(float(v) for v in RO.origin_at((-2.5, 0.1, 3.0), (16, 7, -64), 0.125))
    assert rolling.origin_at((0.1, 0.2, 0.3), (0, 0, 0), 0.05) == tuple(float(np.float32(v)) for v in (0.1, 0.2, 0.3))
