"""scsfm_hip.confidence (libscsfm_conf.so) on the device against tests/confidence_oracle.py, bit for bit: the cases of
tests/_conf_cases.py, which tests/test_confidence_hostsim.py runs on the host simulator -- the pair records, the weights,
the weighted integration (a weight of all ones against libscsfm_fuse's own kernels); then what only the device shows --
guard bands behind the outputs, the Python layer and its refusals, the generated world with a moving object through
scsfm_hip.confidence, and reconstruct.py --consistency-weight end to end."""
import os
import re

import numpy as np
import pytest
import torch

import _conf_cases as C
import confidence_oracle as CO

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 64
f32 = np.float32


def _dev(a, dtype=None):
    return torch.from_numpy(np.array(a, dtype)).to(DEV)   # (np.array copies: the cases are read-only)


def _guarded(count, dtype=torch.float32):
    return torch.full((count + GUARD,), float("nan"), dtype=dtype, device=DEV)


class Backend:
    """the library's entry points on device tensors; the outputs have GUARD elements of NaN behind them, which must stay
    as they were, and the inputs must keep their bits"""

    @staticmethod
    def pairs(c2w, K, radius):
        from scsfm_hip import _lib
        from scsfm_hip.fusion import _ptr, _stream
        c, Kd = _dev(np.asarray(c2w, np.float64).reshape(-1, 12)), _dev(K, np.float32)
        n = len(c)
        out = _guarded(n * 2 * radius * 16)
        _lib.get_conf().call("scsfm_conf_pairs", n, radius, _ptr(c), _ptr(Kd), _ptr(out), _stream(c.device))
        assert bool(torch.isnan(out[n * 2 * radius * 16:]).all()), "pairs: guard"
        assert C.same_bits(c.cpu().numpy(), np.asarray(c2w, np.float64).reshape(-1, 12))
        return out[:n * 2 * radius * 16].reshape(n, 2 * radius, 16).cpu().numpy()

    @staticmethod
    def weights(depth, pair, is_disp=True, max_depth=10.0, min_views=1, floor=0.0, reduce="mean", shift=0):
        """``shift``: the depth and the weights start that many floats into their buffers (off the 16-byte alignment)"""
        from scsfm_hip import _lib
        from scsfm_hip.fusion import _ptr, _stream
        n, H, W = depth.shape
        size = n * H * W
        buf = torch.zeros(size + shift, dtype=torch.float32, device=DEV)
        d = buf[shift:]
        d.copy_(_dev(depth, np.float32).reshape(-1))
        p = _dev(pair, np.float32)
        out = _guarded(size + shift)
        _lib.get_conf().call("scsfm_conf_weights", n, pair.shape[1] // 2, H, W, _ptr(d), int(bool(is_disp)), _ptr(p),
                             float(f32(max_depth)), int(min_views), float(f32(floor)), CO.REDUCE[reduce], _ptr(out[shift:]),
                             _stream(d.device))
        assert bool(torch.isnan(out[size + shift:]).all()) and bool(torch.isnan(out[:shift]).all()), "weights: guard"
        assert C.same_bits(d.cpu().numpy().reshape(depth.shape), np.asarray(depth, np.float32))
        assert C.same_bits(p.cpu().numpy(), np.asarray(pair, np.float32))
        return out[shift:shift + size].reshape(n, H, W).cpu().numpy()

    @staticmethod
    def volume(dims, origin, voxel, trunc, max_weight, frames_per_launch):
        from scsfm_hip import fusion
        return fusion.Volume(dims, origin, voxel, trunc, max_weight, device=DEV, frames_per_launch=frames_per_launch)

    dev = staticmethod(lambda a: _dev(a))
    host = staticmethod(lambda t: t.cpu().numpy())


@pytest.mark.parametrize("name", C.NAMES)
def test_weights_equal_the_oracle_bit_for_bit(name):
    C.check(name, Backend)


@pytest.mark.parametrize("name", C.FUSE_NAMES)
def test_integration_equals_the_oracle_bit_for_bit(name):
    """Volume.integrate(weight=) at F, 2 and 1 frames a launch and as F calls of one frame; a weight of all ones also
    against the unweighted call, the real libscsfm_fuse path, over all five planes"""
    C.check_fuse(name, Backend)


def test_unaligned_buffers_take_the_scalar_path_and_give_the_same_bits():
    """W = 20 is a multiple of 4, but buffers that start 4 bytes off a 16-byte boundary cannot be read 16 bytes at a time"""
    name = "n5_r2_w4_disp"
    case = C.cases()[name]
    pair, weight, _ = C.reference(name)
    for shift in (1, 2, 3):
        assert C.same_bits(Backend.weights(case["depth"], pair, shift=shift, **case["kw"]), weight), shift


@pytest.mark.parametrize("kind", ("rigid", "skewed"))
def test_pairs_equal_the_oracle(kind):
    c2w = C.pair_poses()[kind]
    for radius in (1, 2, 4):
        got, want = Backend.pairs(c2w, C.K_ODD, radius), CO.pairs(c2w, C.K_ODD, radius)
        assert C.same_bits(got, want)
        absent = want[:, :, 12] == 0
        assert absent.any() and not got[absent].view(np.uint32).any()


def test_identical_frames_at_identical_poses_weigh_exactly_one():
    from scsfm_hip import confidence
    for name in ("identical", "identical_pow2"):
        case = C.cases()[name]
        _, _, count = C.reference(name)
        got = confidence.weights(_dev(case["depth"]), _dev(case["c2w"]), _dev(case["K"]), radius=1, **case["kw"]).cpu().numpy()
        assert (got[count > 0] == f32(1)).all() and not got[count == 0].any() and (count > 0).sum() > 500


def test_python_layer_equals_the_oracle_and_refuses():
    from scsfm_hip import confidence, fusion
    case = C.cases()["max_floor_disp"]
    pair, weight, _ = C.reference("max_floor_disp")
    d, c2w, K = _dev(case["depth"]), _dev(case["c2w"]), _dev(case["K"])
    kw = dict(radius=2, is_disp=True, max_depth=C.MAX_DEPTH, min_views=2, floor=0.99, reduce="max")
    got = confidence.weights(d[:, None].contiguous(), c2w, K, **kw)
    assert got.shape == (5,) + C.HW and got.dtype == torch.float32 and C.same_bits(got.cpu().numpy(), weight)
    assert C.same_bits(confidence.weights(d, c2w.reshape(5, 12), K, **kw).cpu().numpy(), weight)
    assert C.same_bits(confidence.pair_cameras(c2w, K, 2).cpu().numpy(), pair)
    with pytest.raises(TypeError, match="HIP device"):
        confidence.weights(d.cpu(), c2w, K)
    with pytest.raises(TypeError, match="float32"):
        confidence.weights(d.double(), c2w, K)
    with pytest.raises(TypeError, match="float64"):
        confidence.weights(d, c2w.float(), K)
    with pytest.raises(ValueError, match="contiguous"):
        confidence.weights(d.transpose(1, 2), c2w, K)
    with pytest.raises(ValueError, match="contiguous"):
        confidence.weights(d, c2w, K.t())
    with pytest.raises(ValueError, match="poses for"):
        confidence.weights(d, c2w[:4].contiguous(), K)
    with pytest.raises(ValueError):
        confidence.weights(d[0], c2w, K)
    for radius in (0, 5, -1):
        with pytest.raises(ValueError, match="radius"):
            confidence.weights(d, c2w, K, radius=radius)
        with pytest.raises(ValueError, match="radius"):
            confidence.pair_cameras(c2w, K, radius)
    with pytest.raises(ValueError, match="reduce"):
        confidence.weights(d, c2w, K, reduce="median")
    for bad in (dict(floor=-0.1), dict(floor=1.5), dict(floor=float("nan")), dict(min_views=0), dict(max_depth=0.0)):
        with pytest.raises(Exception, match="rejected argument"):
            confidence.weights(d, c2w, K, **bad)
    fc = C.fuse_cases()["fractional_scalar_plain"]
    vol = fusion.Volume(fc["dims"], fc["origin"], fc["voxel"], device=DEV)
    call = fc["call"]
    depth, poses, Kf, w = _dev(call["depth"]), _dev(call["c2w"]), _dev(call["K"]), _dev(fc["weight"])
    with pytest.raises(TypeError, match="HIP device"):
        vol.integrate(depth, None, poses, Kf, is_disp=False, weight=w.cpu())
    with pytest.raises(TypeError, match="float32"):
        vol.integrate(depth, None, poses, Kf, is_disp=False, weight=w.double())
    with pytest.raises(ValueError, match="contiguous"):
        vol.integrate(depth, None, poses, Kf, is_disp=False, weight=w.transpose(1, 2))
    with pytest.raises(ValueError, match="weight must be"):
        vol.integrate(depth, None, poses, Kf, is_disp=False, weight=w[:4].contiguous())
    assert not vol.planes.any()      # (a refused call touches nothing)
    vol.integrate(depth, None, poses, Kf, is_disp=False, near=call["near"], max_depth=call["max_depth"], weight=w[:, None].contiguous())
    assert C.same_bits(vol.planes.cpu().numpy(), C.fuse_reference("fractional_scalar_plain").planes)


def test_confidence_does_its_job_on_the_device():
    """tests/test_confidence_hostsim.py's generated world with an object that comes towards the cameras, through
    scsfm_hip.confidence and Volume.integrate(weight=): the weights, the medians and the four point counts are the
    oracle's, so its conditions hold here -- they are asserted again on what the device gave.

    Measured (the oracle and the MI355X agree bit for bit): medians 0.959177 on the plates and 0.995635 on the static
    pixels, floor 0.977406; points inside the object's swept box 104 unweighted and 0 weighted, outside it 2257 and 2164."""
    from scsfm_hip import confidence, fusion
    w, m = C.moving_world(), C.moving_reference()
    depth, c2w, K = _dev(w["depth"]), _dev(w["c2w"]), _dev(w["K"])
    got = confidence.weights(depth, c2w, K, radius=1, is_disp=False, max_depth=C.MAX_DEPTH).cpu().numpy()
    assert C.same_bits(got, m["weight"])
    on, off = C.moving_medians(got, m["count"])
    cut = confidence.weights(depth, c2w, K, radius=1, is_disp=False, max_depth=C.MAX_DEPTH, floor=m["floor"])
    assert C.same_bits(cut.cpu().numpy(), m["cut"])
    counts = []
    for weight in (None, cut):
        vol = fusion.Volume(C.MOVING["dims"], C.MOVING["origin"], C.MOVING["voxel"], device=DEV)
        vol.integrate(depth, None, c2w, K, is_disp=False, near=0.05, max_depth=C.MAX_DEPTH, weight=weight)
        counts.append(C.moving_counts(vol.extract(C.MOVING["min_weight"])[0].cpu().numpy()))
    print(f"medians: plates {on:.6f}, static {off:.6f}; points (inside, outside): unweighted {counts[0]}, weighted {counts[1]}")
    assert on < off and on < m["floor"] < off
    assert counts[1][0] < counts[0][0] and counts[1][1] >= 0.9 * counts[0][1]
    assert tuple(counts) == (m["plain"], m["weighted"])


def _files(folder):
    return sorted(os.listdir(str(folder)))


def test_reconstruct_consistency_weight_on_six_generated_frames(tmp_path, capsys):
    """reconstruct.py --consistency-weight on six generated 64 x 96 frames with randomly initialised nets saved by the test
    (the setting of tests/test_gpu_tracking.py's end-to-end test: this is about plumbing and determinism).  A plain run
    writes exactly poses.txt and reconstruction.ply.  With --consistency-weight --output-confidence poses.txt keeps its
    bytes; the hook's weights equal the oracle on the hook's disparities and the chain's poses, bit for bit;
    confidence.npy and the pictures are those weights; every fused batch is rows of the stored disparities and the
    returned volume equals a fresh one integrated from the hooks' tensors with weight=; the printed line matches numpy
    to 1e-9; a second run writes the same files.  With --refine-poses added the weights keep their bits and the volume
    is again the batches with their rows of the weights."""
    from PIL import Image

    import models
    import reconstruct
    from scsfm_hip import fusion
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
    flags = ["--consistency-weight", "--consistency-radius", "2", "--consistency-floor", "0.5", "--output-confidence"]
    runs = {}
    # (two runs of the nets give the same predictions only with MIOpen's reproducible solvers, as smoke() asks for them)
    old = torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = True, False
    try:
        plain_vol = reconstruct.main(argv + ["--output-dir", str(tmp_path / "plain")])
        plain_out = capsys.readouterr().out
        for name, extra in (("a", flags), ("b", flags), ("refined", flags + ["--refine-poses", "--refine-group", "2"])):
            seen = {"batches": [], "weights": []}
            vol = reconstruct.main(argv + extra + ["--output-dir", str(tmp_path / name)],
                                   on_batch=lambda *t, s=seen: s["batches"].append([x.clone() for x in t]),
                                   on_weights=lambda w, d, s=seen: s["weights"].append((w.clone(), d.clone())))
            runs[name] = (vol, seen, capsys.readouterr().out)
        for bad in (["--consistency-radius", "2"], ["--consistency-weight", "--consistency-radius", "5"]):
            with pytest.raises(SystemExit, match="--consistency-radius"):
                reconstruct.main(argv + bad + ["--output-dir", str(tmp_path / "bad")])
    finally:
        torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = old
    plain = tmp_path / "plain"
    assert _files(plain) == ["poses.txt", "reconstruction.ply"] and not (tmp_path / "bad").exists()
    assert "confidence" not in plain_out and "disparities" not in plain_out
    chain = np.loadtxt(str(plain / "poses.txt"))
    names = [f"{k:06d}" for k in range(6)]
    want = None
    for name, (vol, seen, printed) in runs.items():
        out = tmp_path / name
        assert _files(out) == ["confidence", "confidence.npy", "poses.txt"] + (["poses_refined.txt"] if name == "refined" else []) \
            + ["reconstruction.ply"]
        assert (out / "poses.txt").read_bytes() == (plain / "poses.txt").read_bytes()
        assert _files(out / "confidence") == [n + ".png" for n in names]
        (weight, disp), = seen["weights"]
        assert weight.shape == (6, 64, 96) and disp.shape == (6, 1, 64, 96) and weight.dtype == torch.float32
        K = seen["batches"][0][3]
        if want is None:
            # the chain's poses, as the plain loop hands them to on_batch; they are what poses.txt holds
            c2w = torch.cat([b[2] for b in seen["batches"]]).cpu().numpy()
            assert np.array_equal(np.array([["%1.8e" % v for v in row] for row in c2w.reshape(-1, 12)], float), chain)
            want = CO.weights(disp[:, 0].cpu().numpy(), CO.pairs(c2w, K.cpu().numpy(), 2), is_disp=True, max_depth=2.0,
                              min_views=1, floor=0.5, reduce="mean")
            print(f"weights: mean {want.mean():.6f}, {(want == 0).mean():.6f} at zero, largest {want.max():.6f}")
            first = (weight, disp)
        assert C.same_bits(weight.cpu().numpy(), want), name
        assert torch.equal(weight.view(torch.int32), first[0].view(torch.int32)) and torch.equal(disp, first[1]), name
        assert C.same_bits(np.load(str(out / "confidence.npy")), want)
        grey = (want * f32(255) + f32(0.5)).astype(np.uint8)
        for k, n in enumerate(names):
            assert np.array_equal(np.array(Image.open(str(out / "confidence" / (n + ".png")))), grey[k]), (name, n)
        # every fused batch is rows of the stored disparities, fused with the same rows of the weights
        sizes = [len(b[0]) for b in seen["batches"]]
        assert sizes == ([1, 2, 2, 1] if name == "refined" else [4, 2])
        fresh = fusion.Volume(vol.dims, vol.origin, vol.voxel, vol.trunc, device=DEV, frames_per_launch=2)
        at = 0
        for batch in seen["batches"]:
            assert torch.equal(batch[0], disp[at:at + len(batch[0])])
            fresh.integrate(*batch, is_disp=True, max_depth=2.0, weight=weight[at:at + len(batch[0])])
            at += len(batch[0])
        assert at == 6 and torch.equal(fresh.planes.view(torch.int32), vol.planes.view(torch.int32)), name
        line = [ln for ln in printed.splitlines() if ln.startswith("confidence of ")]
        assert len(line) == 1 and "disparities of 6 frames kept on the device: 0.1 MB" in printed
        m = re.fullmatch(r"confidence of 6 frames: mean (\S+), (\S+) of the pixels at zero", line[0])
        assert m, line[0]
        assert float(m.group(1)) == pytest.approx(want.astype(np.float64).mean(), rel=1e-9, abs=1e-12)
        assert float(m.group(2)) == pytest.approx((want == 0).mean(), rel=1e-9, abs=1e-12)
    # the weights change what is fused, and two runs give the same files
    assert not torch.equal(runs["a"][0].planes, plain_vol.planes)
    for path in ("confidence.npy", "poses.txt", "reconstruction.ply", "confidence/000003.png"):
        assert (tmp_path / "a" / path).read_bytes() == (tmp_path / "b" / path).read_bytes(), path
