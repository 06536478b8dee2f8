"""Snippet pose evaluation on the MI355X (scsfm_hip.snippets over libscsfm_snip.so) against the numpy oracle
(tests/pose_snippet_oracle.py) and the reference's recorded results (tests/golden/pose_snippets.npz), with the
judgement of tests/_pose_snippet_check.py (the same as on the simulator), and test_pose.py end to end, in-process.  The
oracle is fed this package's pose_vec2mat of the vectors, computed on the device and lifted to double (the library
restates its closed forms), so that numpy's sin / cos are not part of the comparison."""
import os
import sys

import numpy as np
import pytest
import torch

import _pose_snippet_check as C
import pose_snippet_oracle as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARIANTS = [(mode, dt) for mode in ("euler", "quat") for dt in ("f32", "f64")]

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "pose_snippets.npz"))


def _eval(*a, **k):
    from scsfm_hip.snippets import evaluate_snippets
    return evaluate_snippets(*a, **k)


def _mats(vecs, mode):
    from inverse_warp import pose_vec2mat
    return [pose_vec2mat(torch.from_numpy(v).cuda(), mode).double().cpu().numpy() if len(v) else np.zeros((0, 3, 4))
            for v in vecs]


def _check(res, vecs, gts, mode, L=5, report=None):
    want = P.evaluate(_mats(vecs, mode), gts, L)
    C.check_errors(res.errors, want["errors"], report)
    C.check_pred(res.predictions, want["pred"])
    C.check_gt(res.gt, want["gt"], gts, L)
    np.testing.assert_allclose(np.concatenate([res.mean, res.std]), P.stats(want["errors"]), rtol=1e-12, atol=0)
    return want


@pytest.mark.parametrize("mode,dt", VARIANTS, ids=[f"{m}-{d}" for m, d in VARIANTS])
def test_fixture_against_oracle_and_golden(golden, mode, dt):
    vecs, gts = [golden[f"vec_{mode}_{dt}_{n}"] for n in "ab"], [golden["gt_a"], golden["gt_b"]]
    res = _eval(vecs, gts, 5, mode)
    assert res.errors.shape == (134, 2) and res.predictions.shape == res.gt.shape == (134, 5, 3, 4)
    report = []
    _check(res, vecs, gts, mode, report=report)
    ref = np.concatenate([golden[f"mean_{mode}_{dt}"], golden[f"std_{mode}_{dt}"]]).astype(np.float64)
    print(report, "stats", res.mean, res.std, "reference", ref)
    np.testing.assert_allclose(np.concatenate([res.mean, res.std]), ref, rtol=1e-5, atol=0)
    C.check_gt(res.gt, golden["gt_comp"], gts, 5)
    if dt == "f64":
        C.check_errors(res.errors, golden[f"errors_{mode}_{dt}"])
    assert res.report_lines() == P.report_lines(ref[:2], ref[2:])


def test_ragged_set_repeat_residence_and_grouping(golden):
    vecs, gts = C.ragged_set(np.float32)
    a = _eval(vecs, gts)
    assert len(a.errors) == 0 + 0 + 1 + 2 + 64 + 65 + 256 + 257
    _check(a, vecs, gts, "euler")
    b = _eval(vecs, gts)
    c = _eval([torch.from_numpy(v).cuda() for v in vecs], [torch.from_numpy(g).cuda().view(-1, 3, 4) for g in gts])
    for x in (b, c):
        for k in ("errors", "predictions", "gt", "mean", "std"):
            assert getattr(a, k).tobytes() == getattr(x, k).tobytes(), k
    at = 0
    for v, g in zip(vecs, gts):
        n = max(len(g) - 4, 0)
        if n:
            one = _eval([v], [g])
            for k in ("errors", "predictions", "gt"):
                assert getattr(one, k).tobytes() == getattr(a, k)[at:at + n].tobytes(), k
        at += n


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("mode", ["euler", "quat"])
def test_second_pose_is_the_inverse_of_pose_vec2mat(golden, mode, dt):
    vecs = [golden[f"vec_{mode}_{dt}_b"]]
    res = _eval(vecs, [golden["gt_b"]], 5, mode)
    want = P.invert(_mats(vecs, mode)[0])[:len(res.errors)]
    np.testing.assert_allclose(res.predictions[:, 1], want, rtol=1e-12, atol=1e-15)
    eye = np.eye(4)[:3]
    assert (res.predictions[:, 0] == eye).all()


@pytest.mark.parametrize("seq_len", [3, 7])
def test_other_snippet_lengths(golden, seq_len):
    vecs, gts = [golden["vec_euler_f32_a"]], [golden["gt_a"]]
    res = _eval(vecs, gts, seq_len)
    assert res.predictions.shape == (69 - seq_len + 1, seq_len, 3, 4)
    _check(res, vecs, gts, "euler", seq_len)


def test_bad_arguments_raise(golden):
    v, g = golden["vec_euler_f32_a"], golden["gt_a"]
    with pytest.raises(ValueError):
        _eval([v], [g[:-1]])           # 68 vectors need 69 poses
    with pytest.raises(ValueError):
        _eval([v, v], [g])
    with pytest.raises(ValueError):
        _eval([v[:3]], [g[:4]])        # four frames: no snippet of five
    with pytest.raises(ValueError):
        _eval([v], [g], rotation_mode="axis")


def _make_tree(tmp_path, golden):
    from PIL import Image

    import models
    torch.manual_seed(0)
    net = models.PoseResNet(18, False)
    ckpt = tmp_path / "pose.pth.tar"
    torch.save({"epoch": 1, "state_dict": net.state_dict()}, ckpt)
    rng = np.random.default_rng(41)
    arrays = {}
    (tmp_path / "poses").mkdir()
    for seq, n, lo in (("09", 7, 0), ("10", 5, 20)):
        d = tmp_path / "sequences" / seq / "image_2"
        d.mkdir(parents=True)
        arrays[seq] = [(rng.random((128, 416, 3)) * 255).astype(np.uint8) for _ in range(n)]
        for i, a in enumerate(arrays[seq]):
            Image.fromarray(a).save(d / f"{i:06d}.png")
        np.savetxt(tmp_path / "poses" / f"{seq}.txt", np.load(os.path.join(ROOT, "tests", "golden", "odom_eval.npz"))
                   ["gt_04"][lo:lo + n], delimiter=' ', fmt='%.17e')
    return net, ckpt, arrays


def test_test_pose_cli(tmp_path, golden, capsys, monkeypatch):
    import models
    import test_pose
    from inverse_warp import pose_vec2mat
    net, ckpt, arrays = _make_tree(tmp_path, golden)
    samples = []
    made = models.PoseResNet

    def counted(*a, **k):
        m = made(*a, **k)
        m.register_forward_hook(lambda mod, inp, out: samples.append(len(out)))
        return m

    monkeypatch.setattr(models, "PoseResNet", counted)
    common = [str(ckpt), "--img-height", "128", "--img-width", "416", "--dataset-dir", str(tmp_path), "--sequences",
              "09", "10"]
    test_pose.main(common + ["--output-dir", str(tmp_path / "b1")])
    out = capsys.readouterr().out.splitlines()
    assert "4 snippets to test" in out
    assert sum(samples) == (7 - 1) + (5 - 1) and len(samples) == 10  # every distinct pair once, not 4 per snippet (16)
    at = out.index("Results")
    assert out[at - 1] == "" and out[at + 1] == "\t {:>10}, {:>10}".format("ATE", "RE")
    mean, std = out[at + 2], out[at + 3]
    assert mean.startswith("mean \t ") and std.startswith("std \t ")
    p1 = np.load(tmp_path / "b1" / "predictions.npy")
    assert p1.shape == (4, 5, 3, 4) and p1.dtype == np.float64 and (p1[:, 0] == np.eye(4)[:3]).all()

    del samples[:]
    test_pose.main(common + ["--output-dir", str(tmp_path / "b4"), "--batch-size", "4"])
    capsys.readouterr()
    assert sum(samples) == 10 and len(samples) == 2 + 1
    p4 = np.load(tmp_path / "b4" / "predictions.npy")
    # batch 4 runs other convolution shapes (MIOpen may pick other kernels): equal up to fp32 reassociation, at the rtol
    # of test_test_vo_cli_writes_the_folded_trajectory
    np.testing.assert_allclose(p4, p1, rtol=1e-4, atol=0)

    # the reference's loop, restated with this package's pose_vec2mat and the oracle's fold, pair by pair
    net = net.cuda().eval()
    want, errs = [], []
    gts = {s: np.loadtxt(tmp_path / "poses" / f"{s}.txt").reshape(-1, 3, 4) for s in arrays}
    with torch.no_grad():
        for seq in ("09", "10"):
            xs = [(torch.from_numpy(a.astype(np.float32).transpose(2, 0, 1)).unsqueeze(0).cuda() / 255 - 0.45) / 0.225
                  for a in arrays[seq]]
            for j in range(len(xs) - 4):
                mats = [pose_vec2mat(net(xs[j + i], xs[j + i + 1])).squeeze(0).double().cpu().numpy() for i in range(4)]
                pred = P.fold(P.invert(np.stack(mats))[None])
                want.append(pred[0])
                errs.append(P.pose_errors(P.compensate(gts[seq][None, j:j + 5]), pred)[0])
    np.testing.assert_allclose(p1, np.stack(want), rtol=1e-4, atol=0)
    m, s = P.stats(np.stack(errs))[:2], P.stats(np.stack(errs))[2:]
    for line, vals in ((mean, m), (std, s)):
        got = [float(x) for x in line.split("\t")[1].split(",")]
        np.testing.assert_allclose(got, vals, rtol=1e-3, atol=1e-4)  # (four printed decimals)

    with pytest.raises(SystemExit):
        test_pose.main(common + ["--sequence-length", "4"])
    assert "--sequence-length" in capsys.readouterr().err


def test_build_resolves_the_snippet_entry_points(capsys):
    sys.path.insert(0, ROOT)
    import __graft_entry__ as G
    G.build()
    out = capsys.readouterr().out.splitlines()
    from scsfm_hip import _lib, build
    tails = [line.split("/")[-1] for line in out if line.startswith("[build] ")]
    headers = [("libscsfm_hip.so", _lib.HEADER), ("libscsfm_nets.so", _lib.NETS_HEADER),
               ("libscsfm_eval.so", _lib.EVAL_HEADER), ("libscsfm_odom.so", _lib.ODOM_HEADER),
               ("libscsfm_enc.so", _lib.ENC_HEADER), ("libscsfm_stem.so", _lib.STEM_HEADER),
               ("libscsfm_snip.so", _lib.SNIP_HEADER)]
    assert tails == [f"{name}: {len(_lib.parse_header(h))} entry points resolved" for name, h in headers]
    assert tails[3] == "libscsfm_odom.so: 7 entry points resolved" and tails[6] == "libscsfm_snip.so: 4 entry points resolved"
    assert _lib.get_snip().source_id() == build.snip_source_id()
