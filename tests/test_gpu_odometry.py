"""Visual odometry on the MI355X (scsfm_hip.odometry over libscsfm_odom.so) against the numpy oracle
(tests/odom_eval_oracle.py) and the reference's recorded results (tests/golden/odom_eval.npz), with the judgement of
tests/_odom_eval_check.py (the same as on the simulator), and the two CLIs end to end."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _odom_eval_check as C
import odom_eval_oracle as O
from test_odom_eval_hostsim import NAMES, synthetic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "sc-sfmlearner-release_amd")

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "odom_eval.npz"))


def _sets(d):
    return [d["gt_04"], d["gt_10"]], [d["pred_04"], d["pred_10"]]


def _as_out(res):
    """An OdomEvalResult in the shape tests/_odom_eval_check.py judges."""
    S = len(res.segments)
    seg = np.zeros((S, max(max(len(s) for s in res.segments), 1), 5))
    for i, s in enumerate(res.segments):
        seg[i, :len(s)] = s
    return dict(summary=res.summary, per_length=res.per_length, seg=seg,
                n_seg=np.array([len(s) for s in res.segments]), gt_rel=[g.reshape(-1, 12) for g in res.gt_rel],
                aligned=[a.reshape(-1, 12) for a in res.aligned])


def _eval(*a, **k):
    from scsfm_hip.odometry import evaluate_odometry
    return evaluate_odometry(*a, **k)


@pytest.mark.parametrize("alignment", O.ALIGNMENTS, ids=str)
def test_fixtures_against_oracle_and_golden(golden, alignment):
    gts, preds = _sets(golden)
    res = _eval(gts, preds, alignment, seqs=[4, 10])
    C.check_set(_as_out(res), gts, preds, alignment)
    name = NAMES[alignment]
    for s, seq in enumerate((4, 10)):
        want = golden[f"seg_{name}_{seq:02}"]
        assert res.segments[s].shape == want.shape
        np.testing.assert_array_equal(res.segments[s][:, [0, 3, 4]], want[:, [0, 3, 4]])
    # the reference's text: result.txt (3 decimals) and the "For Copying" block as they are, the console's 17-digit
    # floats as numbers
    assert res.result_txt() == str(golden[f"result_{name}"])
    want = str(golden[f"stdout_{name}"]).splitlines()
    got = res.report_lines() + res.copy_block()
    assert len(got) == len(want) and got[-5:] == want[-5:]
    for a, b in zip(got, want):
        ha, _, va = a.rpartition("  ")
        hb, _, vb = b.rpartition("  ")
        if ha and ha == hb:
            assert float(va) == pytest.approx(float(vb), rel=1e-9), (a, b)
        else:
            assert a == b
    if alignment == "7dof":
        for s, seq in enumerate((4, 10)):
            ours, ref = res.segment_errors(s).splitlines(), str(golden[f"errors_{name}_{seq:02}"]).splitlines()
            assert len(ours) == len(ref)
            for a, b in zip(ours, ref):
                a, b = a.split(" "), b.split(" ")
                assert (a[0], a[3], a[4]) == (b[0], b[3], b[4])


def test_general_inverse_not_a_transpose(golden):
    gts, preds = _sets(golden)
    res = _eval(gts[1:], preds[1:], None)
    np.testing.assert_allclose(res.summary[0][0], golden["summary_none"][1][0], rtol=1e-10, atol=0)
    np.testing.assert_allclose(res.segments[0][:, 2], golden["seg_none_10"][:, 2], rtol=1e-10, atol=0)


@pytest.mark.parametrize("alignment", O.ALIGNMENTS, ids=str)
def test_synthetic_ragged_sets(alignment):
    gts, preds = synthetic()
    res = _eval(gts, preds, alignment)
    C.check_set(_as_out(res), gts, preds, alignment)


def test_repeat_chunking_and_residence_give_the_same_bytes(golden):
    gts, preds = _sets(golden)
    sg, sp = synthetic()
    gts, preds = [gts[0]] + sg + [gts[1]], [preds[0]] + sp + [preds[1]]
    for alignment in (None, "7dof"):
        a = _eval(gts, preds, alignment)
        b = _eval([torch.from_numpy(g).cuda() for g in gts], [torch.from_numpy(p).cuda().view(-1, 3, 4) for p in preds],
                  alignment)
        for s in range(len(gts)):
            one = _eval(gts[s:s + 1], preds[s:s + 1], alignment)
            for x, y, z in ((a.summary[s], b.summary[s], one.summary[0]),
                            (a.per_length[s], b.per_length[s], one.per_length[0]),
                            (a.segments[s], b.segments[s], one.segments[0]),
                            (a.aligned[s], b.aligned[s], one.aligned[0]), (a.gt_rel[s], b.gt_rel[s], one.gt_rel[0])):
                assert x.tobytes() == y.tobytes() == z.tobytes()


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("mode", ["euler", "quat"])
def test_chain_poses(dtype, mode):
    """The local matrices are exactly this package's pose_vec2mat (the same closed forms, compiled with the same
    flags); the chain against the sequential fold of the kernel's own matrices to n eps max|position|."""
    from inverse_warp import pose_vec2mat
    from scsfm_hip.odometry import chain_poses, chain_poses_ragged
    g = torch.Generator().manual_seed(7)
    vecs = []
    for n in (0, 1, 64, 257, 1590, 4660):
        v = torch.randn((n, 6), generator=g, dtype=torch.float64) * 0.01
        v[:, 2] -= 0.4
        vecs.append(v.to(dtype).cuda())
    poses, local = chain_poses_ragged(vecs, mode, return_local=True)
    report = []
    for v, p, l in zip(vecs, poses, local):
        assert p.dtype == torch.float64 and p.shape == (len(v) + 1, 3, 4) and l.dtype == dtype
        if len(v):
            want = pose_vec2mat(v, mode)
            assert torch.equal(l, want)
        C.check_chain(p.cpu().numpy(), l.cpu().numpy(), report)
        single = chain_poses(v, mode)
        assert single.cpu().numpy().tobytes() == p.cpu().numpy().tobytes()
    print(report)
    again = chain_poses_ragged([v.cpu().numpy() for v in vecs], mode)
    for a, b in zip(poses, again):
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()


def _run(cmd, timeout, cwd=PKG):
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([PKG, ROOT]))
    r = subprocess.run([sys.executable, *cmd], cwd=cwd, env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return r.stdout


def test_test_vo_cli_writes_the_folded_trajectory(tmp_path):
    from PIL import Image

    import models
    from inverse_warp import pose_vec2mat

    torch.manual_seed(0)
    net = models.PoseResNet(18, False)
    ckpt = tmp_path / "pose.pth.tar"
    torch.save({"epoch": 1, "state_dict": net.state_dict()}, ckpt)
    rng = np.random.default_rng(31)
    imgs = tmp_path / "sequences" / "09" / "image_2"
    imgs.mkdir(parents=True)
    arrays = []
    for i in range(6):
        a = (rng.random((128, 416, 3)) * 255).astype(np.uint8)
        Image.fromarray(a).save(imgs / f"{i:06d}.png")
        arrays.append(a)
    common = ["test_vo.py", "--pretrained-posenet", str(ckpt), "--img-height", "128", "--img-width", "416",
              "--dataset-dir", str(tmp_path / "sequences") + "/", "--sequence", "09"]
    out = _run(common + ["--output-dir", str(tmp_path / "b1") + "/"], 600)
    assert "6 files to test" in out
    _run(common + ["--output-dir", str(tmp_path / "b4") + "/", "--batch-size", "4"], 600)
    text = open(tmp_path / "b1" / "09.txt").read().splitlines()
    assert len(text) == 6 and all(len(line.split(" ")) == 12 for line in text)
    assert text[0] == " ".join("%1.8e" % v for v in np.eye(4)[:3].ravel())
    p1 = np.loadtxt(tmp_path / "b1" / "09.txt")
    p4 = np.loadtxt(tmp_path / "b4" / "09.txt")
    # batch 4 runs other convolution shapes (MIOpen may pick other kernels): equal up to fp32 reassociation, at the
    # rtol of test_test_disp_cli_writes_the_models_inverse_disparity
    np.testing.assert_allclose(p4, p1, rtol=1e-4, atol=0)

    net = net.cuda().eval()
    mats = []
    with torch.no_grad():
        xs = [(torch.from_numpy(a.astype(np.float32).transpose(2, 0, 1)).unsqueeze(0).cuda() / 255 - 0.45) / 0.225
              for a in arrays]
        for x0, x1 in zip(xs[:-1], xs[1:]):
            mats.append(pose_vec2mat(net(x0, x1)).squeeze(0).cpu().numpy())
    want = O.fold(np.stack(mats)).reshape(-1, 12)
    # (another process, another batch size: MIOpen may pick other kernels -- the same rtol, for the same reason)
    np.testing.assert_allclose(p1, want, rtol=1e-4, atol=0)


def test_eval_odom_cli_reproduces_the_reference_files(tmp_path, golden):
    res_dir, gt_dir = tmp_path / "vo", tmp_path / "gt"
    res_dir.mkdir(), gt_dir.mkdir()
    for seq in (4, 10):
        np.savetxt(gt_dir / f"{seq:02}.txt", golden[f"gt_{seq:02}"], delimiter=' ', fmt='%.17e')
        np.savetxt(res_dir / f"{seq:02}.txt", golden[f"pred_{seq:02}"], delimiter=' ', fmt='%1.8e')
    out = _run(["kitti_eval/eval_odom.py", "--result", str(res_dir), "--align", "7dof", "--gt-dir", str(gt_dir), "--yes"],
               600)
    lines = [l for l in out.splitlines() if "matplotlib" not in l]
    want = str(golden["stdout_7dof"]).splitlines()
    assert len(lines) == len(want) and lines[-5:] == want[-5:]
    for a, b in zip(lines, want):
        ha, _, va = a.rpartition("  ")
        hb, _, vb = b.rpartition("  ")
        if ha and ha == hb:
            assert float(va) == pytest.approx(float(vb), rel=1e-9), (a, b)
        else:
            assert a == b
    assert open(res_dir / "result.txt").read() == str(golden["result_7dof"])
    for seq in (4, 10):
        ours = np.loadtxt(res_dir / "errors" / f"{seq:02}.txt")
        np.testing.assert_array_equal(ours[:, [0, 3, 4]], golden[f"seg_7dof_{seq:02}"][:, [0, 3, 4]])
    # without --yes the prompt is the reference's, and anything but "y" evaluates nothing
    r = subprocess.run([sys.executable, "kitti_eval/eval_odom.py", "--result", str(res_dir), "--gt-dir", str(gt_dir)],
                       cwd=PKG, input="n\n", capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, PYTHONPATH=os.pathsep.join([PKG, ROOT])))
    assert r.returncode == 0 and "Evaluate result in" in r.stdout and "Double check the path!" in r.stdout


def test_build_resolves_the_odometry_entry_points(capsys):
    sys.path.insert(0, ROOT)
    import __graft_entry__ as G
    G.build()
    out = capsys.readouterr().out
    assert "libscsfm_odom.so: 7 entry points resolved" in out
    from scsfm_hip import _lib
    assert _lib.get_odom().source_id() == __import__("scsfm_hip.build", fromlist=["x"]).odom_source_id()
