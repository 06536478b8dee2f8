"""reconstruct.py's handling of --refine-scale and --refine-scale-pivot, where no device is needed: a flag without the one
it needs and a bad value are refused at the top of main, before the device check; good ones end as the program always ends
without a HIP device; and the Python layer's constant is the header's default."""
import pytest
import torch

import reconstruct

BASE = ["--pretrained-dispnet", "none.pth.tar", "--pretrained-posenet", "none.pth.tar", "--dataset-dir", "none",
        "--intrinsics", "none.txt"]


def test_flags_and_defaults():
    args = reconstruct.parser.parse_args(BASE)
    assert args.refine_scale is False and args.refine_scale_pivot is None
    args = reconstruct.parser.parse_args(BASE + ["--refine-poses", "--refine-scale", "--refine-scale-pivot", "0.01"])
    assert args.refine_poses is True and args.refine_scale is True and args.refine_scale_pivot == 0.01
    from scsfm_hip import similarity
    assert similarity.MIN_SCALE_PIVOT == 2e-3 and similarity.MAX_ITERATIONS == 64
    assert similarity.Track._fields == ("c2w", "scale", "report", "model_depth", "model_normal", "state")
    for flag in ("--refine-scale", "--refine-scale-pivot", "scales_refined.txt", "scsfm_hip.similarity"):
        assert flag in reconstruct.__doc__, flag


@pytest.mark.parametrize("flags, message", [
    (["--refine-scale"], "--refine-scale needs --refine-poses"),
    (["--refine-scale", "--refine-scale-pivot", "0.01"], "--refine-scale needs --refine-poses"),
    (["--refine-scale-pivot", "0.01"], "--refine-scale-pivot needs --refine-scale"),
    (["--refine-poses", "--refine-scale-pivot", "0.01"], "--refine-scale-pivot needs --refine-scale"),
    (["--refine-poses", "--refine-scale", "--refine-scale-pivot", "0"], "--refine-scale-pivot must be positive"),
    (["--refine-poses", "--refine-scale", "--refine-scale-pivot", "-0.002"], "--refine-scale-pivot must be positive"),
    (["--refine-poses", "--refine-scale", "--refine-scale-pivot", "nan"], "--refine-scale-pivot must be positive"),
    (["--refine-poses", "--refine-scale", "--refine-scale-pivot=-inf"], "--refine-scale-pivot must be positive")])
def test_refusals_come_before_the_device_check(flags, message, monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(SystemExit) as e:
        reconstruct.main(BASE + flags)
    assert str(e.value) == message


def test_good_values_without_a_device(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    for flags in (["--refine-poses", "--refine-scale"], ["--refine-poses", "--refine-scale", "--refine-scale-pivot", "0.01"],
                  ["--refine-poses", "--refine-scale", "--refine-scale-pivot", "inf", "--refine-group", "4", "--render"],
                  ["--refine-poses", "--refine-scale", "--consistency-weight"],
                  ["--refine-poses", "--refine-scale", "--follow", "--voxel-size", "0.05"]):
        with pytest.raises(SystemExit, match="needs a HIP device"):
            reconstruct.main(BASE + flags)


def test_python_layer_refuses_host_tensors_without_a_device():
    """the refusals that need no device: a CPU tensor is refused before any library is loaded"""
    from scsfm_hip import similarity
    d, g, s = torch.zeros(2, 4, 6), torch.zeros(2, 3, 4, dtype=torch.float64), torch.ones(2, dtype=torch.float64)
    K, ref = torch.eye(3), torch.zeros(2, 16)
    with pytest.raises(TypeError, match="HIP device"):
        similarity.align(d, g, s, K, ref, d, torch.zeros(2, 3, 4, 6), max_dist=0.3)
    with pytest.raises(TypeError, match="HIP device"):
        similarity.scaled_depth(d, s)
    rep = torch.tensor([[[9.0, 0, 1, 0, 0, 1]] * 2, [[9.0, 0, 3, 0, 0, 1], [9.0, 0, 2, 0, 0, 1]],
                        [[9.0, 0, 3, 0, 0, 1], [9.0, 0, 0, 0, 0, 1]], [[9.0, 0, 2, 0, 0, 1]] * 2], dtype=torch.float64)
    assert similarity.kept_guess(rep).tolist() == [True, False, False, True]
    assert similarity.held_scale(rep).tolist() == [True, True, False, True]
