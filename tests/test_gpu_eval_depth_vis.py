"""eval_depth.py --vis_dir end to end on the GPU on a generated set per dataset (KITTI ragged, one prediction with mean
-1): the decoded PNGs equal the oracle's composites and the metrics printout is the same with and without --vis_dir."""
import os

import numpy as np
import pytest

import _depth_vis_cli as W
import depth_eval_oracle as E
import depth_vis_oracle as O
import eval_depth as ED
from scsfm_hip import depth_vis

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("dataset,gdt,pdt", (("kitti", np.float32, np.float64), ("nyu", np.float32, np.float32),
                                             ("nyu", np.float64, np.float32)), ids=("kitti", "nyu", "nyu-gt64"))
def test_written_pictures_equal_the_oracle(tmp_path, capsys, monkeypatch, dataset, gdt, pdt):
    s = W.write_set(str(tmp_path), dataset, gdt, pdt)
    ED.main(s["argv"])
    plain = capsys.readouterr().out
    assert "abs_rel" in plain
    monkeypatch.setattr(ED, "VIS_CHUNK_PIXELS", 2 * s["sizes"][0][0] * s["sizes"][0][1])  # two pictures, then one
    out = str(tmp_path / "results")
    res = ED.main(s["argv"] + ["--img_dir", s["img"], "--vis_dir", out])
    cap = capsys.readouterr()
    assert cap.out == plain and "1 predictions were skipped" in cap.err
    assert res.evaluated.tolist() == [True, True, False, True]
    names, got = W.read_pictures(os.path.join(out, "vis_depth"))
    assert names == ["0000.png", "0001.png", "0002.png"]
    # the oracle's ratios are the library's, bit for bit (tests/test_gpu_depth_eval.py), so the pictures must agree
    ratios = E.evaluate(s["gts"], s["pred"], dataset)["ratio"]
    assert np.array_equal(ratios[res.evaluated], res.ratio[res.evaluated])
    want = O.composites(s["gts"], s["pred"], ratios, dataset, s["photos"], depth_vis.MAGMA)
    for k in range(3):
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), k
