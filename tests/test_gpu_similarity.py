"""scsfm_hip.similarity (libscsfm_sim3.so) on the device against tests/sim3_oracle.py, bit for bit on the states, their
records, the fp32 scales, the poses, the scales, every report row and the slab of partial sums: the cases of
tests/_sim3_cases.py, which tests/test_similarity_hostsim.py runs on the host simulator; the cross-library check against
libscsfm_track.so on the device; the streaming scale; then what only the device shows -- guard bands behind every output,
similarity.track against similarity.align on its own cast, the Python layer's refusals, and reconstruct.py --refine-scale
end to end."""
import re

import numpy as np
import pytest
import torch

import _sim3_cases as SC
import _track_cases as TC
import sim3_oracle as SO

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 64


def _dev(a, dtype):
    return torch.from_numpy(np.array(a, dtype)).to(DEV)   # (np.array copies: the cases are read-only)


def _out(count, dtype):
    return torch.full((count + GUARD,), float("nan"), dtype=dtype, device=DEV)


class Backend:
    """the library's entry points on device tensors; every output has GUARD elements of NaN behind it, which must stay as
    they were"""

    @staticmethod
    def align(depth, guess, scale0, K, ref_view, model_depth, model_normal, is_disp, near, max_depth, iterations, max_dist,
              min_pairs, min_scale_pivot):
        from scsfm_hip import _lib
        from scsfm_hip.raycast import _ptr, _stream
        lib = _lib.get_sim3()
        V, H, W = depth.shape
        d, g, s0 = _dev(depth, np.float32), _dev(guess, np.float64), _dev(scale0, np.float64)
        Kd, ref = _dev(K, np.float32), _dev(ref_view, np.float32)
        M, N = _dev(model_depth, np.float32), _dev(model_normal, np.float32)
        n_ws = lib.size("scsfm_sim3_ws_bytes", V, H, W) // 8
        assert n_ws == V * -(-H * W // 1024) * 37
        state, est, sigma_f = _out(8 * V, torch.float64), _out(16 * V, torch.float32), _out(V, torch.float32)
        ws, report = _out(n_ws, torch.float64), _out(6 * V * iterations, torch.float64)
        c2w, scale = _out(12 * V, torch.float64), _out(V, torch.float64)
        stream = _stream(d.device)
        lib.call("scsfm_sim3_init", V, _ptr(g), _ptr(s0), _ptr(Kd), _ptr(state), _ptr(est), _ptr(sigma_f), stream)
        lib.call("scsfm_sim3_iterate", V, H, W, _ptr(d), int(bool(is_disp)), float(np.float32(near)),
                 float(np.float32(max_depth)), _ptr(ref), _ptr(M), _ptr(N), float(np.float32(max_dist)), int(min_pairs),
                 float(min_scale_pivot), int(iterations), _ptr(state), _ptr(est), _ptr(sigma_f), _ptr(ws), _ptr(report),
                 stream)
        lib.call("scsfm_sim3_poses", V, _ptr(state), _ptr(c2w), _ptr(scale), stream)
        got = {}
        for key, t, count, shape in (("state", state, 8 * V, (V, 8)), ("est", est, 16 * V, (V, 16)),
                                     ("sigma_f", sigma_f, V, (V,)), ("slab", ws, n_ws, (V, -1, 37)),
                                     ("report", report, 6 * V * iterations, (V, iterations, 6)),
                                     ("c2w", c2w, 12 * V, (V, 3, 4)), ("scale", scale, V, (V,))):
            assert bool(torch.isnan(t[count:]).all()), f"{key}: guard"
            got[key] = t[:count].reshape(shape).cpu().numpy()
        for t, want in ((d, depth), (s0, scale0), (ref, ref_view), (M, model_depth), (N, model_normal)):
            assert TC.same_bits(t.cpu().numpy(), want)      # (the inputs are only read)
        return got


class TrackBackend:
    """libscsfm_track.so on the device, as tests/test_gpu_tracking.py calls it"""

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
        state, est, ws = _out(7 * V, torch.float64), _out(16 * V, torch.float32), _out(n_ws, torch.float64)
        report, c2w = _out(4 * V * iterations, torch.float64), _out(12 * V, torch.float64)
        stream = _stream(d.device)
        lib.call("scsfm_track_init", V, _ptr(g), _ptr(Kd), _ptr(state), _ptr(est), stream)
        lib.call("scsfm_track_iterate", V, H, W, _ptr(d), int(bool(is_disp)), float(np.float32(near)),
                 float(np.float32(max_depth)), _ptr(ref), _ptr(M), _ptr(N), float(np.float32(max_dist)), int(min_pairs),
                 int(iterations), _ptr(state), _ptr(est), _ptr(ws), _ptr(report), stream)
        lib.call("scsfm_track_poses", V, _ptr(state), _ptr(c2w), stream)
        return dict(state=state[:7 * V].reshape(V, 7).cpu().numpy(), est=est[:16 * V].reshape(V, 16).cpu().numpy(),
                    c2w=c2w[:12 * V].reshape(V, 3, 4).cpu().numpy(),
                    report=report[:4 * V * iterations].reshape(V, iterations, 4).cpu().numpy())


@pytest.mark.parametrize("name", SC.NAMES)
def test_case_equals_the_oracle_bit_for_bit(name):
    SC.check(name, Backend)


@pytest.mark.parametrize("name", TC.NAMES)
def test_rigid_step_equals_the_track_library_bit_for_bit(name):
    """scale0 = 1 and min_scale_pivot = inf: the pose part of the state, the record, the c2w and the report's count, sum
    of r r and pose pivot ratio are libscsfm_track.so's own, status 0 there being 3 here"""
    SC.check_against_track(name, Backend, TrackBackend)


@pytest.mark.parametrize("shape", [(3, 12, 20), (3, 37, 61), (1, 1, 1), (2, 1, 3), (1, 5, 13)])
def test_scale_equals_numpys_product_bit_for_bit(shape):
    """the 16-byte path, its scalar tail, the scalar path of pointers off a 16-byte boundary and frames whose boundary
    falls inside a group of four; NaN, zeros, denormals and infinities among the inputs; the guard behind the output"""
    from scsfm_hip import _lib
    from scsfm_hip.raycast import _ptr, _stream
    rng = np.random.default_rng(5)
    depth = rng.uniform(0.2, 5.0, shape).astype(np.float32)
    if depth.size >= 9:
        depth.reshape(-1)[:6] = (np.nan, 0.0, -0.0, 1e-45, 3e-39, np.inf)
        depth.reshape(-1)[-3:] = (-2.0, 3e38, 1e-30)
    sigma_f = np.array([1.05, 0.93, 1e-39][:shape[0]], np.float32)
    V, H, W = shape
    n = depth.size
    for is_disp in (False, True):
        want = SO.scaled_depth(depth, sigma_f, is_disp)
        for offset in (0, 1, 2):
            src = torch.zeros(n + offset, dtype=torch.float32, device=DEV)
            src[offset:] = _dev(depth, np.float32).reshape(-1)
            out = torch.full((offset + n + GUARD,), float("nan"), dtype=torch.float32, device=DEV)
            s = _dev(sigma_f, np.float32)
            d, o = src[offset:], out[offset:]
            assert d.data_ptr() % 16 == 4 * offset and o.data_ptr() % 16 == 4 * offset
            _lib.get_sim3().call("scsfm_sim3_scale", V, H, W, _ptr(d), int(is_disp), _ptr(s), _ptr(o), _stream(d.device))
            assert TC.same_bits(o[:n].reshape(shape).cpu().numpy(), want), (is_disp, offset)
            assert bool(torch.isnan(out[:offset]).all()) and bool(torch.isnan(o[n:]).all())
            assert TC.same_bits(d.cpu().numpy(), depth.reshape(-1))


def _room_volume():
    from scsfm_hip import fusion
    planes = TC.room_planes()
    _, nz, ny, nx = planes.shape
    vol = fusion.Volume((nx, ny, nz), TC.ORIGIN, TC.VOXEL, device=DEV)
    vol.planes.copy_(torch.from_numpy(np.array(planes, np.float32)))
    return vol


def test_track_equals_align_on_its_own_cast_and_the_oracle():
    """Volume.track_scaled casts the guesses exactly as Volume.track does and aligns to that cast: the same bits as
    similarity.align on the maps it returns, and as the oracle on them; scaled_depth is the oracle's product"""
    from scsfm_hip import raycast, similarity
    case = SC.cases()["perturbed"]["args"]
    vol = _room_volume()
    depth, guess, K = _dev(case["depth"], np.float32), _dev(case["guess"], np.float64), _dev(case["K"], np.float32)
    scale0 = _dev(case["scale0"], np.float64)
    kwargs = dict(is_disp=False, near=0.05, max_depth=TC.MAX_DEPTH, iterations=4, min_pairs=24)
    got = vol.track_scaled(depth, guess, scale0, K, **kwargs)
    assert isinstance(got, similarity.Track) and got.c2w.shape == (3, 3, 4) and got.c2w.dtype == torch.float64
    assert got.scale.shape == (3,) and got.scale.dtype == torch.float64 and got.state.shape == (3, 8)
    assert got.report.shape == (3, 4, 6)
    rigid = vol.track(depth, guess, K, **kwargs)
    assert torch.equal(rigid.model_depth.view(torch.int32), got.model_depth.view(torch.int32))
    assert torch.equal(rigid.model_normal.view(torch.int32), got.model_normal.view(torch.int32))
    ref_view = raycast.views(guess, K)
    again = similarity.align(depth[:, None], guess, scale0, K, ref_view, got.model_depth, got.model_normal,
                             max_dist=vol.trunc, **kwargs)
    want = SO.align(case["depth"], case["guess"], case["scale0"], case["K"], ref_view.cpu().numpy(),
                    got.model_depth.cpu().numpy(), got.model_normal.cpu().numpy(), max_dist=vol.trunc, **kwargs)
    for t in (got, again):
        assert TC.same_bits(t.c2w.cpu().numpy(), want["c2w"]) and TC.same_bits(t.report.cpu().numpy(), want["report"])
        assert TC.same_bits(t.state.cpu().numpy(), want["state"]) and TC.same_bits(t.scale.cpu().numpy(), want["scale"])
    # (so that the comparison is not one of frames that never moved: every iteration solved, and after four of them on
    # maps cast from the guesses themselves, at 12 x 20, every scale is nearer the depth's factor of 1.05 than its start)
    assert (want["report"][:, :, 2] == 0).all() and np.abs(want["scale"] - 1.05).max() < 0.025
    assert not bool(similarity.kept_guess(got.report).any()) and not bool(similarity.held_scale(got.report).any())
    # never solved: the rigid tracker's poses, bit for bit
    held = vol.track_scaled(depth, guess, scale0, K, min_scale_pivot=float("inf"), **kwargs)
    assert torch.equal(held.c2w, rigid.c2w) and similarity.held_scale(held.report).tolist() == [True] * 3
    assert not bool(similarity.kept_guess(held.report).any()) and torch.equal(held.scale, scale0)
    away = guess.clone()
    away[1] = _dev(SC.cases()["looks_away"]["args"]["guess"][1], np.float64)
    lost = vol.track_scaled(depth, away, scale0, K, **kwargs)
    assert similarity.kept_guess(lost.report).tolist() == [False, True, False]
    assert similarity.held_scale(lost.report).tolist() == [False, True, False]
    # the scaled depth, in both layouts
    scaled = similarity.scaled_depth(depth, got.scale, is_disp=False)
    want_d = SO.scaled_depth(case["depth"], want["scale"].astype(np.float32), False)
    assert scaled.shape == depth.shape and TC.same_bits(scaled.cpu().numpy(), want_d)
    assert torch.equal(similarity.scaled_depth(depth[:, None], got.scale, is_disp=False), scaled[:, None])


def test_python_layer_refusals():
    from scsfm_hip import similarity
    case = SC.cases()["perturbed"]["args"]
    vol = _room_volume()
    depth, guess, K = _dev(case["depth"], np.float32), _dev(case["guess"], np.float64), _dev(case["K"], np.float32)
    s0 = _dev(case["scale0"], np.float64)
    ref, M, N = _dev(case["ref_view"], np.float32), _dev(case["model_depth"], np.float32), _dev(case["model_normal"], np.float32)
    kw = dict(is_disp=False, max_depth=4.0, max_dist=0.3)
    with pytest.raises(TypeError, match="HIP device"):
        vol.track_scaled(depth.cpu(), guess, s0, K, is_disp=False)
    with pytest.raises(TypeError, match="float32"):
        vol.track_scaled(depth.double(), guess, s0, K, is_disp=False)
    with pytest.raises(TypeError, match="float64"):
        vol.track_scaled(depth, guess.float(), s0, K, is_disp=False)
    with pytest.raises(TypeError, match="float64"):
        vol.track_scaled(depth, guess, s0.float(), K, is_disp=False)
    with pytest.raises(TypeError, match="HIP device"):
        vol.track_scaled(depth, guess, s0.cpu(), K, is_disp=False)
    with pytest.raises(ValueError, match="contiguous"):
        vol.track_scaled(depth.transpose(1, 2), guess, s0, K, is_disp=False)
    with pytest.raises(ValueError, match="contiguous"):
        similarity.align(depth, guess, s0, K.t(), ref, M, N, **kw)
    with pytest.raises(ValueError, match="contiguous"):
        similarity.align(depth, guess, torch.ones(6, dtype=torch.float64, device=DEV)[::2], K, ref, M, N, **kw)
    with pytest.raises(TypeError, match="HIP device"):
        similarity.align(depth, guess, s0, K, ref, M.cpu(), N, **kw)
    with pytest.raises(ValueError):
        similarity.align(depth, guess[:2].contiguous(), s0, K, ref, M, N, **kw)
    with pytest.raises(ValueError):
        similarity.align(depth, guess, s0[:2].contiguous(), K, ref, M, N, **kw)
    with pytest.raises(ValueError):
        similarity.align(depth, guess, s0, K, ref, M, N[:, :2].contiguous(), **kw)
    for bad in (dict(iterations=0), dict(iterations=65), dict(min_pairs=6), dict(min_scale_pivot=0.0),
                dict(min_scale_pivot=-1.0), dict(min_scale_pivot=float("nan"))):
        with pytest.raises(ValueError):
            similarity.align(depth, guess, s0, K, ref, M, N, **kw, **bad)
    for bad in (dict(max_dist=0.0), dict(max_dist=float("nan")), dict(max_depth=-1.0), dict(near=-0.1)):
        with pytest.raises(Exception, match="rejected argument"):
            similarity.align(depth, guess, s0, K, ref, M, N, **{**kw, **bad})
    with pytest.raises(ValueError):
        similarity.scaled_depth(depth, s0[:2].contiguous(), is_disp=False)
    with pytest.raises(TypeError, match="float64"):
        similarity.scaled_depth(depth, s0.float(), is_disp=False)


def _files(folder):
    import os
    return sorted(os.listdir(str(folder)))


def test_reconstruct_refine_scale_on_six_generated_frames(tmp_path, capsys):
    """reconstruct.py --refine-poses --refine-scale on six generated 64 x 96 frames with randomly initialised nets saved by
    the test (the nets of tests/test_gpu_tracking.py; they track badly or not at all: this is about plumbing and
    determinism).  Without the flag --refine-poses writes and prints what it does, and no scales; with the flag and a
    scale that is never solved (--refine-scale-pivot inf) every file and line of that run keeps its bytes; with the flag
    poses.txt keeps its bytes; row 0 of scales_refined.txt is 1; every tracked group starts from the scale of the frame
    fused before it and equals the oracle's align on the hook's own tensors, bit for bit; every fused batch is the scaled
    depth at the refined pose; the returned volume equals a fresh one integrated from those; the printed lines match numpy
    on the hooks' reports to 1e-9; and --refine-group 2 passes the same checks."""
    from PIL import Image

    import models
    import reconstruct
    from scsfm_hip import fusion, raycast, similarity
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
            "--frames-per-launch", "2", "--refine-iterations", "3", "--refine-poses"]
    runs, rigid = {}, {}
    # (two runs of the nets give the same predictions only with MIOpen's reproducible solvers, as smoke() asks for them)
    old = torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = True, False
    try:
        for k, flags in enumerate(([], ["--refine-scale", "--refine-scale-pivot", "inf"])):
            reconstruct.main(argv + flags + ["--output-dir", str(tmp_path / f"rigid{k}")])
            rigid[k] = capsys.readouterr().out.replace(f"rigid{k}", "rigid")
        for group in (1, 2):
            seen = {"batches": [], "tracks": []}
            vol = reconstruct.main(argv + ["--refine-scale", "--refine-group", str(group), "--output-dir",
                                           str(tmp_path / f"g{group}")],
                                   on_batch=lambda *t, s=seen: s["batches"].append([x.clone() for x in t]),
                                   on_track=lambda ids, guess, got, disp, s=seen: s["tracks"].append(
                                       (list(ids), guess.clone(), got, disp.clone())))
            runs[group] = (vol, seen, capsys.readouterr().out)
    finally:
        torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = old
    # without the flag: what --refine-poses writes and prints, and no file of the scales; with the flag and a scale that
    # is never solved (a pivot of inf) the same bytes in every file and line, beside scales of 1 that were all held
    assert _files(tmp_path / "rigid0") == ["poses.txt", "poses_refined.txt", "reconstruction.ply"]
    for name in _files(tmp_path / "rigid0"):
        assert (tmp_path / "rigid0" / name).read_bytes() == (tmp_path / "rigid1" / name).read_bytes(), name
    assert (tmp_path / "rigid1" / "scales_refined.txt").read_text() == "1.00000000e+00\n" * 6
    assert "scales_refined" not in rigid[0]
    never = rigid[1].splitlines()
    (k,) = [i for i, ln in enumerate(never) if ln.startswith("refined 5 scales ")]
    assert never[k].endswith("scales_refined.txt: min 1, mean 1, max 1, 5 frames held their scale throughout")
    assert never[:k] + never[k + 1:] == rigid[0].splitlines()
    chain_bytes = (tmp_path / "rigid0" / "poses.txt").read_bytes()
    for group, (vol, seen, printed) in runs.items():
        out = tmp_path / f"g{group}"
        assert _files(out) == ["poses.txt", "poses_refined.txt", "reconstruction.ply", "scales_refined.txt"]
        assert (out / "poses.txt").read_bytes() == chain_bytes
        # the lines printed are those of --refine-poses with one more, directly behind its own
        mine = [ln.replace(f"g{group}", "rigid") for ln in printed.splitlines()]
        extra = [i for i, ln in enumerate(mine) if ln.startswith("refined 5 scales ")]
        assert len(extra) == 1 and mine[extra[0] - 1].startswith("refined 5 poses ")
        assert len(mine) == len(rigid[0].splitlines()) + 1
        text =(out / "scales_refined.txt").read_text().splitlines()
        assert len(text) == 6 and text[0] == "1.00000000e+00"
        scales = np.loadtxt(str(out / "scales_refined.txt"))
        refined = np.loadtxt(str(out / "poses_refined.txt"))
        assert [ids for ids, *_ in seen["tracks"]] == [list(range(k, min(k + group, 6))) for k in range(1, 6, group)]
        assert len(seen["batches"]) == 1 + len(seen["tracks"])
        K = seen["batches"][0][3]
        fresh = fusion.Volume(vol.dims, vol.origin, vol.voxel, vol.trunc, device=DEV, frames_per_launch=2)
        # the first frame: scale 1, untracked; its batch is the depth 1 * (1 / disp), which is positive and finite
        first = seen["batches"][0][0]
        assert first.shape == (1, 1, 64, 96) and bool((first > 0).all()) and bool(torch.isfinite(first).all())
        fresh.integrate(*seen["batches"][0], is_disp=False, max_depth=2.0)
        reports, last, all_scales = [], np.float64(1.0), [1.0]
        for (ids, guess, got, disp), batch in zip(seen["tracks"], seen["batches"][1:]):
            assert isinstance(got, similarity.Track)
            scale0 = torch.full((len(ids),), float(last), dtype=torch.float64, device=DEV)
            mine = fresh.track_scaled(disp, guess, scale0, K, is_disp=True, max_depth=2.0, iterations=3)
            assert torch.equal(mine.c2w, got.c2w) and torch.equal(mine.scale, got.scale)
            assert torch.equal(mine.model_depth.view(torch.int32), got.model_depth.view(torch.int32))
            want = SO.align(disp[:, 0].cpu().numpy(), guess.cpu().numpy(), scale0.cpu().numpy(), K.cpu().numpy(),
                            raycast.views(guess, K).cpu().numpy(), got.model_depth.cpu().numpy(),
                            got.model_normal.cpu().numpy(), is_disp=True, near=0.0, max_depth=2.0, iterations=3,
                            max_dist=vol.trunc, min_pairs=64, min_scale_pivot=2e-3)
            for key in ("c2w", "scale", "report", "state"):
                assert TC.same_bits(getattr(got, key).cpu().numpy(), want[key]), key
            rep = want["report"]
            assert (rep[:, 0, 5] == last).all()              # the group started from the scale of the frame before it
            kept = np.isin(rep[:, :, 2], (1, 2)).all(axis=1)
            poses = np.where(kept[:, None, None], guess.cpu().numpy(), want["c2w"])
            scale = np.where(kept, float(last), want["scale"])
            assert TC.same_bits(batch[2].cpu().numpy(), poses)      # fused at the refined poses, or at the kept guess
            depth = SO.scaled_depth(disp[:, 0].cpu().numpy(), scale.astype(np.float32), True)
            assert TC.same_bits(batch[0].cpu().numpy(), depth[:, None])         # ... from the scaled depth
            assert torch.equal(similarity.scaled_depth(disp, _dev(scale, np.float64), is_disp=True), batch[0])
            assert np.array_equal(np.array([["%1.8e" % v for v in row] for row in poses.reshape(-1, 12)], float),
                                  refined[ids])
            assert np.array_equal(np.array(["%1.8e" % v for v in scale], float), scales[ids])
            fresh.integrate(*batch, is_disp=False, max_depth=2.0)
            reports.append(rep)
            all_scales += scale.tolist()
            last = np.float64(scale[-1])
        assert torch.equal(fresh.planes, vol.planes)
        # the printed lines against numpy on the hooks' reports
        rep = np.concatenate(reports)
        line = [ln for ln in printed.splitlines() if ln.startswith("refined ")]
        assert len(line) == 2
        m = re.fullmatch(r"refined 5 poses -> \S+poses_refined\.txt: mean rms residual (\S+) -> (\S+), mean pair share "
                         r"(\S+), (\d+) frames kept their guess", line[0])
        assert m, line[0]
        for it, text in ((0, m.group(1)), (-1, m.group(2))):
            some = rep[:, it, 0] > 0
            if some.any():
                assert float(text) == pytest.approx(np.sqrt(rep[some, it, 1] / rep[some, it, 0]).mean(), rel=1e-9)
            else:
                assert text == "nan"
        assert float(m.group(3)) == pytest.approx((rep[:, -1, 0] / (64 * 96)).mean(), rel=1e-9)
        assert int(m.group(4)) == np.isin(rep[:, :, 2], (1, 2)).all(axis=1).sum()
        m = re.fullmatch(r"refined 5 scales -> \S+scales_refined\.txt: min (\S+), mean (\S+), max (\S+), (\d+) frames held "
                         r"their scale throughout", line[1])
        assert m, line[1]
        print(f"group {group}: {line[0]}\n{line[1]}")
        tracked = np.array(all_scales[1:])
        for text, value in zip(m.groups()[:3], (tracked.min(), tracked.mean(), tracked.max())):
            assert float(text) == pytest.approx(value, rel=1e-9)
        assert int(m.group(4)) == (rep[:, :, 2] != 0).all(axis=1).sum()
