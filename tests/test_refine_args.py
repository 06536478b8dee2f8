"""reconstruct.py's handling of the --refine-* flags, where no device is needed: bad values are refused at the top of main,
before the device check; good ones end as the program always ends without a HIP device; and the pose algebra of the
guesses, on the CPU."""
import numpy as np
import pytest
import torch

import reconstruct
from _fusion_cases import pose

BASE = ["--pretrained-dispnet", "none.pth.tar", "--pretrained-posenet", "none.pth.tar", "--dataset-dir", "none",
        "--intrinsics", "none.txt"]


def test_flags_and_defaults():
    args = reconstruct.parser.parse_args(BASE)
    assert args.refine_poses is False and args.refine_iterations == 10 and args.refine_group == 1
    assert args.refine_max_dist is None
    args = reconstruct.parser.parse_args(BASE + ["--refine-poses", "--refine-iterations", "4", "--refine-group", "8",
                                                 "--refine-max-dist", "0.2"])
    assert args.refine_poses is True and args.refine_iterations == 4 and args.refine_group == 8
    assert args.refine_max_dist == 0.2


@pytest.mark.parametrize("flags, name", [(["--refine-iterations", "0"], "--refine-iterations"),
                                         (["--refine-iterations", "65"], "--refine-iterations"),
                                         (["--refine-iterations", "-3"], "--refine-iterations"),
                                         (["--refine-group", "0"], "--refine-group"),
                                         (["--refine-group", "-1"], "--refine-group"),
                                         (["--refine-max-dist", "0"], "--refine-max-dist"),
                                         (["--refine-max-dist", "-0.1"], "--refine-max-dist"),
                                         (["--refine-max-dist", "nan"], "--refine-max-dist"),
                                         (["--refine-max-dist", "inf"], "--refine-max-dist")])
def test_bad_values_are_refused_before_the_device_check(flags, name, monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(SystemExit, match=name):
        reconstruct.main(BASE + ["--refine-poses"] + flags)


def test_good_values_without_a_device(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    for flags in (["--refine-poses"], ["--refine-poses", "--refine-iterations", "64", "--refine-group", "8"],
                  ["--refine-poses", "--refine-max-dist", "0.5", "--render"]):
        with pytest.raises(SystemExit, match="needs a HIP device"):
            reconstruct.main(BASE + flags)


def test_relative_to_applies_the_chains_motion_to_the_refined_anchor():
    chain = torch.from_numpy(np.stack([pose(0.1 * k, -0.05 * k, (0.2 * k, 0.1, 0.3 * k)) for k in range(4)]))
    refined = torch.from_numpy(pose(0.12, -0.03, (0.25, 0.08, 0.31)))
    got = reconstruct.relative_to(refined, chain[1], chain[1:])

    def hom(p):
        return np.concatenate([p.numpy(), [[0, 0, 0, 1.0]]])
    assert got.dtype == torch.float64 and got.shape == (3, 3, 4) and got.is_contiguous()
    for k in range(3):
        want = hom(refined) @ np.linalg.inv(hom(chain[1])) @ hom(chain[1 + k])
        assert np.abs(got[k].numpy() - want[:3]).max() < 1e-14
    assert np.abs(got[0].numpy() - refined.numpy()).max() < 1e-15    # the anchor itself lands on its refined pose
    same = reconstruct.relative_to(chain[2], chain[2], chain)          # an anchor that did not move moves nothing
    assert np.abs(same.numpy() - chain.numpy()).max() < 1e-15
