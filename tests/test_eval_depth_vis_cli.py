"""eval_depth.py --vis_dir / --img_dir without a GPU: argument handling, the pairing of pictures with photographs when a
prediction was skipped, file names, size mismatches and too few photographs.  The device functions are substituted by the
numpy oracles (tests/depth_eval_oracle.py, tests/depth_vis_oracle.py), so the written PNGs are checked too."""
import os

import numpy as np
import pytest
import torch
from PIL import Image

import _depth_vis_cli as W
import depth_eval_oracle as E
import depth_vis_oracle as O
import eval_depth as ED
from scsfm_hip import depth_eval, depth_vis


@pytest.fixture
def on_host(monkeypatch):
    calls = []

    def evaluate(gts, pred, dataset, eval_mono=True):
        r = E.evaluate(gts, pred, dataset)
        return depth_eval.DepthEvalResult(dataset, r["metrics"], r["ratio"], r["med_gt"], r["med_pred"], r["count"],
                                          r["flag"] == 1, r["ratios"], r["mean"], r["ratio_stats"])

    def composites(res, pred, gts, dataset, photos, first=0):
        calls.append((first, len(photos)))
        assert all(p.dtype == torch.uint8 for p in photos)
        every = O.composites(gts, pred, res.ratio, dataset, _pad(photos, first, gts, pred), depth_vis.MAGMA)
        return [torch.from_numpy(c) for c in every[first:first + len(photos)]]

    def _pad(photos, first, gts, pred):
        sizes = [np.asarray(gts[i]).shape for i in O.evaluated(pred)]
        out = [np.zeros(s + (3,), np.uint8) for s in sizes]
        for k, p in enumerate(photos):
            out[first + k] = p.numpy()
        return out

    monkeypatch.setattr(depth_eval, "evaluate_depth", evaluate)
    monkeypatch.setattr(depth_vis, "composites", composites)
    monkeypatch.setattr(ED, "DEVICE", "cpu")
    return calls


def test_help_strings_and_vis_dir_alone(capsys):
    help_of = {a.option_strings[0]: a.help for a in ED.parser._actions if a.option_strings}
    assert help_of["--vis_dir"] == "result directory for saving visualization"
    assert help_of["--img_dir"] == "image directory for reading image"
    with pytest.raises(SystemExit) as e:
        ED.main(["--dataset", "kitti", "--pred_depth", "p.npy", "--gt_depth", "gt", "--vis_dir", "out"])
    assert e.value.code == 2 and "--vis_dir needs --img_dir" in capsys.readouterr().err


@pytest.mark.parametrize("dataset", ("kitti", "nyu"))
def test_img_dir_alone_is_ignored(tmp_path, on_host, capsys, dataset):
    s = W.write_set(str(tmp_path), dataset)
    ED.main(s["argv"])
    plain = capsys.readouterr().out
    ED.main(s["argv"] + ["--img_dir", s["img"]])
    assert capsys.readouterr().out == plain and on_host == []
    assert sorted(os.listdir(tmp_path)) == sorted(["gt" if dataset == "kitti" else "gt.npy", "img", "pred.npy"])


@pytest.mark.parametrize("dataset", ("kitti", "nyu"))
def test_pictures_names_and_pairing_with_a_skipped_prediction(tmp_path, on_host, capsys, monkeypatch, dataset):
    s = W.write_set(str(tmp_path), dataset)
    ED.main(s["argv"])
    plain = capsys.readouterr()
    monkeypatch.setattr(ED, "VIS_CHUNK_PIXELS", 2 * s["sizes"][0][0] * s["sizes"][0][1])  # two pictures, then one
    out = str(tmp_path / "results")
    ED.main(s["argv"] + ["--img_dir", s["img"], "--vis_dir", out])
    cap = capsys.readouterr()
    assert cap.out == plain.out  # the printed output is unchanged
    assert cap.err.count("\n") == 1 and "1 predictions were skipped" in cap.err
    assert on_host == [(0, 2), (2, 1)]
    names, got = W.read_pictures(os.path.join(out, "vis_depth"))
    assert names == ["0000.png", "0001.png", "0002.png"]
    ratios = E.evaluate(s["gts"], s["pred"], dataset)["ratio"]
    want = O.composites(s["gts"], s["pred"], ratios, dataset, s["photos"], depth_vis.MAGMA)
    for k, (g, w) in enumerate(zip(got, want)):
        H, W_ = s["sizes"][k]
        assert g.shape == ((H, 3 * W_, 3) if dataset == "nyu" else (2 * H, W_, 3)) and np.array_equal(g, w), k
    # picture 2 shows prediction 3 (prediction 2 was skipped) beside photograph 2
    H, W_ = s["sizes"][2]
    assert np.array_equal(got[2][:H, :W_], s["photos"][2])
    assert depth_vis.evaluated_indices(ED_result(s, dataset)).tolist() == [0, 1, 3]


def ED_result(s, dataset):
    r = E.evaluate(s["gts"], s["pred"], dataset)
    return depth_eval.DepthEvalResult(dataset, r["metrics"], r["ratio"], r["med_gt"], r["med_pred"], r["count"],
                                      r["flag"] == 1, r["ratios"], r["mean"], r["ratio_stats"])


def test_no_warning_without_a_skipped_prediction(tmp_path, on_host, capsys):
    s = W.write_set(str(tmp_path), "nyu", skip=False)
    ED.main(s["argv"] + ["--img_dir", s["img"], "--vis_dir", str(tmp_path / "r")])
    assert capsys.readouterr().err == ""
    assert sorted(os.listdir(tmp_path / "r" / "vis_depth")) == [f"{k:04d}.png" for k in range(4)]


def test_size_mismatch_names_the_file(tmp_path, on_host):
    s = W.write_set(str(tmp_path), "kitti")
    bad = os.path.join(s["img"], f"{1:010d}.png")
    Image.fromarray(np.zeros((36, 121, 3), np.uint8)).save(bad)
    with pytest.raises(SystemExit) as e:
        ED.main(s["argv"] + ["--img_dir", s["img"], "--vis_dir", str(tmp_path / "r")])
    assert bad in str(e.value) and "36 x 121" in str(e.value) and "36 x 122" in str(e.value)


def test_too_few_photographs(tmp_path, on_host):
    s = W.write_set(str(tmp_path), "kitti", n_photos=2)
    with pytest.raises(SystemExit) as e:
        ED.main(s["argv"] + ["--img_dir", s["img"], "--vis_dir", str(tmp_path / "r")])
    assert "3 predictions to visualise but only 2 *.png" in str(e.value)
    assert not (tmp_path / "r").exists()


def test_photographs_are_read_as_opencv_reads_8_bit_files(tmp_path):
    rgb = np.random.default_rng(0).integers(0, 256, (5, 7, 3), dtype=np.uint8)
    Image.fromarray(rgb).save(tmp_path / "rgb.png")
    Image.fromarray(rgb[..., 0]).save(tmp_path / "grey.png")
    rgba = np.concatenate([rgb, np.full((5, 7, 1), 9, np.uint8)], axis=2)
    Image.fromarray(rgba).save(tmp_path / "rgba.png")
    assert np.array_equal(ED.read_photo(str(tmp_path / "rgb.png")), rgb)
    assert np.array_equal(ED.read_photo(str(tmp_path / "grey.png")), np.repeat(rgb[..., :1], 3, axis=2))
    assert np.array_equal(ED.read_photo(str(tmp_path / "rgba.png")), rgb)  # (alpha dropped, as IMREAD_COLOR does)
    assert 1 <= ED.PNG_THREADS <= 16
