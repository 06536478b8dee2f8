"""scsfm_hip.tracking (libscsfm_track.so) on the device against tests/track_oracle.py, bit for bit on the states, their
records, the poses, every report row and the slab of partial sums: the cases of tests/_track_cases.py, which
tests/test_tracking_hostsim.py runs on the host simulator; then what only the device shows -- guard bands behind the slab,
the states, the records and the report, tracking.track against tracking.align on its own cast, the Python layer's
refusals, and reconstruct.py --refine-poses end to end."""
import re

import numpy as np
import pytest
import torch

import _track_cases as TC
import track_oracle as TO

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 64


def _dev(a, dtype):
    return torch.from_numpy(np.array(a, dtype)).to(DEV)   # (np.array copies: the cases are read-only)


class Backend:
    """the library's entry points on device tensors; the states, the records, the slab and the report have GUARD elements
    of NaN behind them, which must stay as they were"""

    @staticmethod
    def align(depth, guess, K, ref_view, model_depth, model_normal, is_disp, near, max_depth, iterations, max_dist,
              min_pairs):
        from scsfm_hip import _lib
        from scsfm_hip.raycast import _ptr, _stream
        lib = _lib.get_track()
        V, H, W = depth.shape
        d, g, Kd, ref = _dev(depth, np.float32), _dev(guess, np.float64), _dev(K, np.float32), _dev(ref_view, np.float32)
        M, N = _dev(model_depth, np.float32), _dev(model_normal, np.float32)
        n_ws = lib.size("scsfm_track_ws_bytes", V, H, W) // 8
        assert n_ws == V * -(-H * W // 1024) * 29

        def out(count, dtype):
            return torch.full((count + GUARD,), float("nan"), dtype=dtype, device=DEV)
        state, est, ws = out(7 * V, torch.float64), out(16 * V, torch.float32), out(n_ws, torch.float64)
        report, c2w = out(4 * V * iterations, torch.float64), out(12 * V, torch.float64)
        stream = _stream(d.device)
        lib.call("scsfm_track_init", V, _ptr(g), _ptr(Kd), _ptr(state), _ptr(est), stream)
        lib.call("scsfm_track_iterate", V, H, W, _ptr(d), int(bool(is_disp)), float(np.float32(near)),
                 float(np.float32(max_depth)), _ptr(ref), _ptr(M), _ptr(N), float(np.float32(max_dist)), int(min_pairs),
                 int(iterations), _ptr(state), _ptr(est), _ptr(ws), _ptr(report), stream)
        lib.call("scsfm_track_poses", V, _ptr(state), _ptr(c2w), stream)
        got = {}
        for key, t, count, shape in (("state", state, 7 * V, (V, 7)), ("est", est, 16 * V, (V, 16)),
                                     ("slab", ws, n_ws, (V, -1, 29)), ("report", report, 4 * V * iterations, (V, iterations, 4)),
                                     ("c2w", c2w, 12 * V, (V, 3, 4))):
            assert bool(torch.isnan(t[count:]).all()), f"{key}: guard"
            got[key] = t[:count].reshape(shape).cpu().numpy()
        for t, want in ((d, depth), (ref, ref_view), (M, model_depth), (N, model_normal)):   # (the inputs are only read)
            assert TC.same_bits(t.cpu().numpy(), want)
        return got


@pytest.mark.parametrize("name", TC.NAMES)
def test_case_equals_the_oracle_bit_for_bit(name):
    TC.check(name, Backend)


def _room_volume():
    from scsfm_hip import fusion
    planes = TC.room_planes()
    _, nz, ny, nx = planes.shape
    vol = fusion.Volume((nx, ny, nz), TC.ORIGIN, TC.VOXEL, device=DEV)
    vol.planes.copy_(torch.from_numpy(np.array(planes, np.float32)))
    return vol


def test_track_equals_align_on_its_own_cast_and_the_oracle():
    """Volume.track casts the guesses (min_weight 1, to max_depth + trunc) and aligns to that cast: the same bits as
    tracking.align on the maps it returns, and as the oracle on them; the python layer's align equals the oracle on the
    "perturbed" case too"""
    from scsfm_hip import raycast, tracking
    case = TC.cases()["perturbed"]["args"]
    vol = _room_volume()
    depth, guess, K = _dev(case["depth"], np.float32), _dev(case["guess"], np.float64), _dev(case["K"], np.float32)
    kwargs = dict(is_disp=False, near=0.05, max_depth=TC.MAX_DEPTH, iterations=4, min_pairs=24)
    got = vol.track(depth, guess, K, **kwargs)
    assert isinstance(got, tracking.Track) and got.c2w.shape == (3, 3, 4) and got.c2w.dtype == torch.float64
    assert got.model_depth.shape == (3, TC.H, TC.W) and got.model_normal.shape == (3, 3, TC.H, TC.W)
    cast = vol.raycast(guess, K, TC.HW, 0.05, TC.MAX_DEPTH + vol.trunc, min_weight=1.0, colour=False, shade=False)
    assert torch.equal(cast.depth.view(torch.int32), got.model_depth.view(torch.int32))
    assert torch.equal(cast.normal.view(torch.int32), got.model_normal.view(torch.int32))
    ref_view = raycast.views(guess, K)
    again = tracking.align(depth[:, None], guess, K, ref_view, got.model_depth, got.model_normal, max_dist=vol.trunc,
                           **kwargs)
    want = TO.align(case["depth"], case["guess"], case["K"], ref_view.cpu().numpy(), got.model_depth.cpu().numpy(),
                    got.model_normal.cpu().numpy(), max_dist=vol.trunc, **kwargs)
    for t in (got, again):
        assert TC.same_bits(t.c2w.cpu().numpy(), want["c2w"]) and TC.same_bits(t.report.cpu().numpy(), want["report"])
        assert TC.same_bits(t.state.cpu().numpy(), want["state"])
    assert (want["report"][:, :, 2] == 0).all() and not bool(tracking.kept_guess(got.report).any())
    away = guess.clone()
    away[1] = _dev(TC.cases()["looks_away"]["args"]["guess"][1], np.float64)
    assert tracking.kept_guess(vol.track(depth, away, K, **kwargs).report).tolist() == [False, True, False]


def test_python_layer_refusals():
    from scsfm_hip import raycast, tracking
    case = TC.cases()["perturbed"]["args"]
    vol = _room_volume()
    depth, guess, K = _dev(case["depth"], np.float32), _dev(case["guess"], np.float64), _dev(case["K"], np.float32)
    ref, M, N = _dev(case["ref_view"], np.float32), _dev(case["model_depth"], np.float32), _dev(case["model_normal"], np.float32)
    kw = dict(is_disp=False, max_depth=4.0, max_dist=0.3)
    with pytest.raises(TypeError, match="HIP device"):
        vol.track(depth.cpu(), guess, K, is_disp=False)
    with pytest.raises(TypeError, match="float32"):
        vol.track(depth.double(), guess, K, is_disp=False)
    with pytest.raises(TypeError, match="float64"):
        vol.track(depth, guess.float(), K, is_disp=False)
    with pytest.raises(ValueError, match="contiguous"):
        vol.track(depth.transpose(1, 2), guess, K, is_disp=False)
    with pytest.raises(ValueError, match="contiguous"):
        tracking.align(depth, guess, K.t(), ref, M, N, **kw)
    with pytest.raises(TypeError, match="HIP device"):
        tracking.align(depth, guess, K, ref, M.cpu(), N, **kw)
    with pytest.raises(ValueError):
        tracking.align(depth, guess[:2].contiguous(), K, ref, M, N, **kw)
    with pytest.raises(ValueError):
        tracking.align(depth, guess, K, ref, M, N[:, :2].contiguous(), **kw)
    for bad in (dict(iterations=0), dict(iterations=65), dict(min_pairs=5)):
        with pytest.raises(ValueError):
            tracking.align(depth, guess, K, ref, M, N, **kw, **bad)
    for bad in (dict(max_dist=0.0), dict(max_dist=float("nan")), dict(max_depth=-1.0), dict(near=-0.1)):
        with pytest.raises(Exception, match="rejected argument"):
            tracking.align(depth, guess, K, ref, M, N, **{**kw, **bad})
    assert raycast.views(guess, K).shape == (3, 16)


def _files(folder):
    import os
    return sorted(os.listdir(str(folder)))


def test_reconstruct_refine_poses_on_six_generated_frames(tmp_path, capsys):
    """reconstruct.py --refine-poses on six generated 64 x 96 frames with randomly initialised nets saved by the test (the
    nets of tests/test_gpu_raycast.py; they track badly or not at all: this is about plumbing and determinism).  With the
    flag poses.txt keeps its bytes; row 0 of poses_refined.txt is row 0 of poses.txt; every tracked group equals the
    oracle's align on the hook's own tensors, bit for bit; the returned volume equals a fresh one integrated from the
    hooks' disparities at the refined poses in the same groups; the printed line matches numpy on the hooks' reports to
    1e-9; and --refine-group 2 passes the same checks."""
    from PIL import Image

    import models
    import reconstruct
    from scsfm_hip import fusion, raycast
    torch.manual_seed(4)
    rng = np.random.default_rng(4)
    frames = tmp_path / "frames"
    frames.mkdir()
    yy, xx = np.mgrid[:64, :96]
    for k in range(6):
        base = 128 + 60 * np.sin((xx + 7 * k) / 9.0)[..., None] * np.cos(yy / 11.0)[..., None]
        Image.fromarray(np.clip(base + rng.normal(0, 12, (64, 96, 3)), 0, 255).astype(np.uint8)).save(
            str(frames / f"{k:06d}.png"))
    torch.save({"state_dict": models.DispResNet(18, False).state_dict()}, str(tmp_path / "disp.pth.tar"))
    torch.save({"state_dict": models.PoseResNet(18, False).state_dict()}, str(tmp_path / "pose.pth.tar"))
    np.savetxt(str(tmp_path / "cam.txt"), np.array([[58.0, 0, 47.5], [0, 58.0, 31.5], [0, 0, 1]]))
    argv = ["--pretrained-dispnet", str(tmp_path / "disp.pth.tar"), "--pretrained-posenet", str(tmp_path / "pose.pth.tar"),
            "--dataset-dir", str(frames), "--intrinsics", str(tmp_path / "cam.txt"), "--img-height", "64", "--img-width",
            "96", "--batch-size", "4", "--max-depth", "2.0", "--resolution", "96", "--min-weight", "1",
            "--frames-per-launch", "2", "--refine-iterations", "3"]
    runs = {}
    # (two runs of the nets give the same predictions only with MIOpen's reproducible solvers, as smoke() asks for them)
    old = torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = True, False
    try:
        reconstruct.main(argv + ["--output-dir", str(tmp_path / "plain")])
        capsys.readouterr()
        for group in (1, 2):
            seen = {"batches": [], "tracks": []}
            vol = reconstruct.main(argv + ["--refine-poses", "--refine-group", str(group), "--output-dir",
                                           str(tmp_path / f"g{group}")],
                                   on_batch=lambda *t, s=seen: s["batches"].append([x.clone() for x in t]),
                                   on_track=lambda ids, guess, got, disp, s=seen: s["tracks"].append(
                                       (list(ids), guess.clone(), got, disp.clone())))
            runs[group] = (vol, seen, capsys.readouterr().out)
    finally:
        torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = old
    plain = tmp_path / "plain"
    assert _files(plain) == ["poses.txt", "reconstruction.ply"]
    chain = np.loadtxt(str(plain / "poses.txt"))
    for group, (vol, seen, printed) in runs.items():
        out = tmp_path / f"g{group}"
        assert _files(out) == ["poses.txt", "poses_refined.txt", "reconstruction.ply"]
        assert (out / "poses.txt").read_bytes() == (plain / "poses.txt").read_bytes()
        text = (out / "poses_refined.txt").read_text().splitlines()
        assert len(text) == 6 and text[0] == (plain / "poses.txt").read_text().splitlines()[0]
        refined = np.loadtxt(str(out / "poses_refined.txt"))
        # the groups: the first frame alone and untracked, then groups of `group`
        assert [ids for ids, *_ in seen["tracks"]] == [list(range(k, min(k + group, 6))) for k in range(1, 6, group)]
        assert len(seen["batches"]) == 1 + len(seen["tracks"])
        K = seen["batches"][0][3]
        assert np.array_equal(np.array(["%1.8e" % v for v in seen["batches"][0][2].reshape(-1).tolist()], float), chain[0])
        fresh = fusion.Volume(vol.dims, vol.origin, vol.voxel, vol.trunc, device=DEV, frames_per_launch=2)
        fresh.integrate(*seen["batches"][0], is_disp=True, max_depth=2.0)
        reports = []
        for (ids, guess, got, disp), batch in zip(seen["tracks"], seen["batches"][1:]):
            assert torch.equal(disp, batch[0])
            # the track is Volume.track on the model fused so far, and the oracle's align on the hook's own tensors
            mine = fresh.track(disp, guess, K, is_disp=True, max_depth=2.0, iterations=3)
            assert torch.equal(mine.c2w, got.c2w) and torch.equal(mine.model_depth.view(torch.int32),
                                                                   got.model_depth.view(torch.int32))
            want = TO.align(disp[:, 0].cpu().numpy(), guess.cpu().numpy(), K.cpu().numpy(),
                            raycast.views(guess, K).cpu().numpy(), got.model_depth.cpu().numpy(),
                            got.model_normal.cpu().numpy(), is_disp=True, near=0.0, max_depth=2.0, iterations=3,
                            max_dist=vol.trunc, min_pairs=64)
            assert TC.same_bits(got.c2w.cpu().numpy(), want["c2w"]) and TC.same_bits(got.report.cpu().numpy(), want["report"])
            assert TC.same_bits(got.state.cpu().numpy(), want["state"])
            rep = want["report"]
            kept = (rep[:, :, 2] != 0).all(axis=1)
            poses = np.where(kept[:, None, None], guess.cpu().numpy(), want["c2w"])
            assert TC.same_bits(batch[2].cpu().numpy(), poses)      # fused at the refined poses, or at the kept guess
            assert np.array_equal(np.array([["%1.8e" % v for v in row] for row in poses.reshape(-1, 12)], float),
                                  refined[ids])
            fresh.integrate(*batch, is_disp=True, max_depth=2.0)
            reports.append(rep)
        assert torch.equal(fresh.planes, vol.planes)
        # the printed line against numpy on the hooks' reports
        rep = np.concatenate(reports)
        line = [ln for ln in printed.splitlines() if ln.startswith("refined ")]
        assert len(line) == 1
        m = re.fullmatch(r"refined 5 poses -> \S+poses_refined\.txt: mean rms residual (\S+) -> (\S+), mean pair share "
                         r"(\S+), (\d+) frames kept their guess", line[0])
        assert m, line[0]
        print(f"group {group}: {line[0]}")
        for it, text in ((0, m.group(1)), (-1, m.group(2))):
            some = rep[:, it, 0] > 0
            if some.any():
                assert float(text) == pytest.approx(np.sqrt(rep[some, it, 1] / rep[some, it, 0]).mean(), rel=1e-9)
            else:
                assert text == "nan"
        assert float(m.group(3)) == pytest.approx((rep[:, -1, 0] / (64 * 96)).mean(), rel=1e-9)
        assert int(m.group(4)) == ((rep[:, :, 2] != 0).all(axis=1)).sum()
