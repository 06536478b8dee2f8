"""Depth evaluation on the MI355X (scsfm_hip.depth_eval over libscsfm_eval.so) against the numpy oracle
(tests/depth_eval_oracle.py) and the reference's recorded results (tests/golden/depth_eval_*.npz), and the two CLIs end to
end.  Medians, ratios, counts and flags must be exact; the metrics agree to 1e-12 relative, except the terms built on
float32 logarithms (the device's logf / log10f against numpy's: see tests/test_depth_eval_hostsim.py for the bound)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _depth_eval_data as D
import depth_eval_oracle as O
from test_depth_eval_hostsim import log_bound

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "sc-sfmlearner-release_amd")

pytestmark = pytest.mark.gpu


def _eval(*a, **k):
    from scsfm_hip.depth_eval import evaluate_depth
    return evaluate_depth(*a, **k)


def _check(res, ref, gd, pd):
    np.testing.assert_array_equal(res.evaluated, ref["flag"] == 1)
    ev = res.evaluated
    np.testing.assert_array_equal(res.count[ev], ref["count"][ev])
    for got, want in ((res.ratio, ref["ratio"]), (res.med_gt, ref["med_gt"]), (res.med_pred, ref["med_pred"])):
        np.testing.assert_array_equal(got, want.astype(np.float64))  # bit-equal to np.median and numpy's division
    for c, name in enumerate(O.COLUMNS):
        atol = log_bound(gd, pd, name == "log10") if name in ("rmse_log", "log10") else 0.0
        np.testing.assert_allclose(res.metrics[ev, c], ref["metrics"][ev, c], rtol=1e-12, atol=atol, err_msg=name)


@pytest.fixture(scope="module")
def kitti():
    return D.kitti_set(24, seed=21)


@pytest.fixture(scope="module")
def nyu():
    return D.nyu_set(16, seed=22)


@pytest.mark.parametrize("pd", [np.float64, np.float32], ids=["pred_f64", "pred_f32"])
def test_kitti_shaped_against_oracle(kitti, pd):
    gts, pred = kitti[0], kitti[1].astype(pd)
    res = _eval(gts, pred, "kitti")
    ref = O.evaluate(gts, pred, "kitti")
    _check(res, ref, np.float32, pd)
    assert 0.005 < res.count.sum() / sum(g.size for g in gts) < 0.04  # (4 % valid before the crop)
    assert res.report_lines() == O.report_lines("kitti", ref["mean"], ref["ratio_stats"])


@pytest.mark.parametrize("pd", [np.float64, np.float32], ids=["pred_f64", "pred_f32"])
def test_nyu_shaped_against_oracle(nyu, pd):
    gts, pred = nyu[0], nyu[1].astype(pd)
    res = _eval(torch.from_numpy(gts).cuda(), torch.from_numpy(pred).cuda(), "nyu")
    ref = O.evaluate(list(gts), pred, "nyu")
    _check(res, ref, np.float32, pd)
    assert res.report_lines() == O.report_lines("nyu", ref["mean"], ref["ratio_stats"])


def test_bit_identical_runs_and_chunks(kitti):
    gts, pred = kitti
    a, b, c = _eval(gts, pred, "kitti"), _eval(gts, pred, "kitti"), _eval(gts, pred, "kitti", chunk=5)
    for k in ("metrics", "ratio", "med_gt", "med_pred", "count", "evaluated"):
        assert getattr(a, k).tobytes() == getattr(b, k).tobytes() == getattr(c, k).tobytes(), k


def test_skipped_and_empty_images():
    gts, pred = D.kitti_set(4, seed=23)
    pred[1] = -1.0
    gts[2][:] = 0.0
    res = _eval(gts, pred, "kitti")
    assert list(res.evaluated) == [True, False, True, True]
    assert res.count[2] == 0 and np.isnan(res.metrics[2]).all() and np.isnan(res.ratio[2])
    assert len(res.ratios) == 3 and np.isnan(res.mean).all()  # (the reference's NaN propagates the same way)


@pytest.mark.parametrize("name", ["kitti", "nyu"])
def test_golden_fixtures_reproduced(name, golden_dir):
    d = np.load(os.path.join(golden_dir, f"depth_eval_{name}.npz"))
    sizes = [tuple(s) for s in d["gt_shapes"]]
    cuts = np.cumsum([h * w for h, w in sizes])[:-1]
    gts = [g.reshape(s) for g, s in zip(np.split(d["gt"], cuts), sizes)]
    pred = d["pred"]
    res = _eval(gts, pred, name)
    np.testing.assert_array_equal(res.ratios, d["ratios"])
    cols = [O.COLUMNS.index(c) for c in O.DATASET_COLUMNS[name]]
    rdt = np.result_type(gts[0].dtype, pred.dtype)
    got, want = res.metrics[res.evaluated][:, cols], d["errors"]
    for j, c in enumerate(O.DATASET_COLUMNS[name]):
        # the reference means in the promoted dtype: float64 -> 1e-12, float32 -> its pairwise sum's rounding
        rtol = 1e-12 if rdt == np.float64 else 1e-5
        atol = log_bound(gts[0].dtype, pred.dtype, c == "log10") if c in ("rmse_log", "log10") else 0.0
        np.testing.assert_allclose(got[:, j], want[:, j], rtol=rtol, atol=atol, err_msg=c)
    assert ["==> Evaluating depth result..."] + res.report_lines() == str(d["stdout"]).splitlines()


def _run(cmd, timeout):
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([PKG, ROOT]))
    r = subprocess.run([sys.executable, *cmd], cwd=PKG, env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return r.stdout


def test_eval_depth_cli_both_datasets(tmp_path, kitti, nyu):
    gts, pred = kitti
    gdir = tmp_path / "kitti_gt"
    gdir.mkdir()
    for i, g in enumerate(gts):
        np.save(gdir / f"{i:06d}.npy", g)
    np.save(tmp_path / "kitti_pred.npy", pred)
    out = _run(["eval_depth.py", "--dataset", "kitti", "--pred_depth", str(tmp_path / "kitti_pred.npy"),
                "--gt_depth", str(gdir), "--ratio_name", str(tmp_path / "ratios.txt")], 300)
    ref = O.evaluate(gts, pred, "kitti")
    want = ["==> Evaluating depth result..."] + O.report_lines("kitti", ref["mean"], ref["ratio_stats"])
    assert out.splitlines() == want
    np.savetxt(tmp_path / "want.txt", ref["ratios"], fmt="%.4f")
    assert (tmp_path / "ratios.txt").read_text() == (tmp_path / "want.txt").read_text()

    ngt, npred = nyu
    np.save(tmp_path / "nyu_gt.npy", ngt)
    np.save(tmp_path / "nyu_pred.npy", npred)
    out = _run(["eval_depth.py", "--dataset", "nyu", "--pred_depth", str(tmp_path / "nyu_pred.npy"),
                "--gt_depth", str(tmp_path / "nyu_gt.npy")], 300)
    ref = O.evaluate(list(ngt), npred, "nyu")
    assert out.splitlines() == ["==> Evaluating depth result..."] + O.report_lines("nyu", ref["mean"],
                                                                                   ref["ratio_stats"])


def test_test_disp_cli_writes_the_models_inverse_disparity(tmp_path):
    from PIL import Image

    import models
    from utils import save_checkpoint

    torch.manual_seed(0)
    net = models.DispResNet(18, False)
    save_checkpoint(tmp_path, {"epoch": 1, "state_dict": net.state_dict()}, {"epoch": 1, "state_dict": {}}, False)
    rng = np.random.default_rng(24)
    imgs = tmp_path / "color"
    imgs.mkdir()
    arrays = []
    for i in range(5):
        a = (rng.random((256, 832, 3)) * 255).astype(np.uint8)
        Image.fromarray(a).save(imgs / f"{i:04d}.png")
        arrays.append(a)
    common = ["test_disp.py", "--pretrained-dispnet", str(tmp_path / "dispnet_checkpoint.pth.tar"), "--resnet-layers",
              "18", "--img-height", "256", "--img-width", "832", "--dataset-dir", str(imgs)]
    out = _run(common + ["--output-dir", str(tmp_path / "b1")], 600)
    assert "5 files to test" in out and "Avg Speed" in out
    _run(common + ["--output-dir", str(tmp_path / "b4"), "--batch-size", "4"], 600)
    p1 = np.load(tmp_path / "b1" / "predictions.npy")
    p4 = np.load(tmp_path / "b4" / "predictions.npy")
    assert p1.dtype == np.float64 and p1.shape == (5, 256, 832)

    # float64 copies of float32 values, as the reference's predictions[j] = 1 / pred_disp
    np.testing.assert_array_equal(p1.astype(np.float32).astype(np.float64), p1)
    # batch 4 runs other convolution shapes (MIOpen may pick other kernels): equal up to fp32 reassociation
    np.testing.assert_allclose(p4, p1, rtol=1e-4, atol=0)

    net = net.cuda().eval()
    want = []
    with torch.no_grad():
        for a in arrays:
            x = torch.from_numpy(a.astype(np.float32).transpose(2, 0, 1)).unsqueeze(0).cuda()
            want.append(1 / net((x / 255 - 0.45) / 0.225).cpu().numpy()[0, 0])
    # the model's own 1 / disp in this process: MIOpen may pick another convolution kernel in another process
    # (measured: 3 % of the entries 1-2 ulp apart), so a few float32 ulp
    np.testing.assert_allclose(p1, np.stack(want).astype(np.float64), rtol=1e-6, atol=0)
