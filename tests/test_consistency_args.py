"""reconstruct.py's handling of the --consistency-* flags, where no device is needed: a flag without --consistency-weight
and a value out of range are refused at the top of main, before the device check; good ones end as the program always
ends without a HIP device."""
import pytest
import torch

import reconstruct

BASE = ["--pretrained-dispnet", "none.pth.tar", "--pretrained-posenet", "none.pth.tar", "--dataset-dir", "none",
        "--intrinsics", "none.txt"]


def test_flags_and_defaults():
    args = reconstruct.parser.parse_args(BASE)
    assert args.consistency_weight is False and args.output_confidence is False
    assert args.consistency_radius is None and args.consistency_reduce is None      # (filled in by main: 1, mean, 1, 0.0)
    assert args.consistency_min_views is None and args.consistency_floor is None
    args = reconstruct.parser.parse_args(BASE + ["--consistency-weight", "--consistency-radius", "3", "--consistency-reduce",
                                                 "max", "--consistency-min-views", "2", "--consistency-floor", "0.5",
                                                 "--output-confidence"])
    assert args.consistency_weight and args.consistency_radius == 3 and args.consistency_reduce == "max"
    assert args.consistency_min_views == 2 and args.consistency_floor == 0.5 and args.output_confidence
    with pytest.raises(SystemExit):
        reconstruct.parser.parse_args(BASE + ["--consistency-weight", "--consistency-reduce", "median"])
    for word in ("--consistency-weight", "--consistency-floor", "confidence.npy", "scsfm_hip.confidence"):
        assert word in reconstruct.__doc__, word


@pytest.mark.parametrize("flags", [["--consistency-radius", "2"], ["--consistency-reduce", "max"],
                                   ["--consistency-reduce", "mean"], ["--consistency-min-views", "1"],
                                   ["--consistency-floor", "0.0"], ["--output-confidence"]])
def test_a_flag_without_consistency_weight_is_refused(flags, monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(SystemExit, match=flags[0] + " needs --consistency-weight"):
        reconstruct.main(BASE + flags)


@pytest.mark.parametrize("flags, name", [(["--consistency-radius", "0"], "--consistency-radius"),
                                         (["--consistency-radius", "5"], "--consistency-radius"),
                                         (["--consistency-radius", "-1"], "--consistency-radius"),
                                         (["--consistency-min-views", "0"], "--consistency-min-views"),
                                         (["--consistency-min-views", "-2"], "--consistency-min-views"),
                                         (["--consistency-floor", "-0.1"], "--consistency-floor"),
                                         (["--consistency-floor", "1.5"], "--consistency-floor"),
                                         (["--consistency-floor", "nan"], "--consistency-floor"),
                                         (["--consistency-floor", "inf"], "--consistency-floor")])
def test_bad_values_are_refused_before_the_device_check(flags, name, monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(SystemExit, match=name + " must"):
        reconstruct.main(BASE + ["--consistency-weight"] + flags)


def test_good_values_without_a_device(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    for flags in (["--consistency-weight"], ["--consistency-weight", "--consistency-radius", "4", "--consistency-floor", "1"],
                  ["--consistency-weight", "--consistency-reduce", "max", "--consistency-min-views", "8", "--refine-poses",
                   "--output-confidence"], []):
        with pytest.raises(SystemExit, match="needs a HIP device"):
            reconstruct.main(BASE + flags)


def test_too_many_pixels_are_refused_with_a_hint_at_every():
    import argparse
    on, off = argparse.Namespace(consistency_weight=True), argparse.Namespace(consistency_weight=False)
    reconstruct.too_many_pixels(on, 10082, (256, 832))          # (the most frames of 256 x 832 whose pixels an int counts)
    assert 10082 * 256 * 832 <= 2 ** 31 - 1 < 10083 * 256 * 832
    with pytest.raises(SystemExit, match="--every"):
        reconstruct.too_many_pixels(on, 10083, (256, 832))
    reconstruct.too_many_pixels(off, 10 ** 6, (256, 832))       # (without the flag nothing is kept)
