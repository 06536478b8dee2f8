"""scsfm_hip.raycast (libscsfm_cast.so) on the device against tests/raycast_oracle.py, bit for bit on the depth, the normals,
the colours and the shade: the cases of tests/_raycast_cases.py, which tests/test_raycast_hostsim.py runs on the host
simulator (the spoiled view records among them passed there first); then what only the device shows -- outputs with guard
rows behind them, the Python layer's defaults and refusals, and reconstruct.py --render end to end."""
import re

import numpy as np
import pytest
import torch

import _raycast_cases as RC
import raycast_oracle as RO

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 64


def _volume(planes, origin, voxel):
    from scsfm_hip import fusion
    _, nz, ny, nx = planes.shape
    vol = fusion.Volume((nx, ny, nz), origin, voxel, device=DEV)
    vol.planes.copy_(torch.from_numpy(np.array(planes, np.float32)))  # (np.array copies: the cases are read-only)
    return vol


class Backend:
    """the library's entry points on device tensors; every output has GUARD elements of fill behind it, which must stay
    as they were"""

    @staticmethod
    def brick_mask(planes, min_weight):
        from scsfm_hip import raycast
        return raycast.brick_mask(_volume(planes, (0, 0, 0), 1.0), min_weight).cpu().numpy().reshape(-1)

    @staticmethod
    def cast(planes, origin, voxel, view, hw, near, step, n_steps, min_weight, mask, normals, colour, shade):
        from scsfm_hip import _lib
        from scsfm_hip.raycast import _ptr, _stream
        vol = _volume(planes, origin, voxel)
        (H, W), V = hw, len(view)
        rec = torch.from_numpy(np.array(view, np.float32)).to(DEV)
        mk = None if mask is None else torch.from_numpy(np.array(mask, np.uint8)).to(DEV)
        n = V * H * W

        def out(count, dtype, fill, want=True):
            return torch.full((count + GUARD,), fill, dtype=dtype, device=DEV) if want else None
        depth, normal = out(n, torch.float32, float("nan")), out(3 * n, torch.float32, float("nan"), normals)
        rgb, sh = out(3 * n, torch.uint8, 0xAB, colour), out(n, torch.uint8, 0xAB, shade)
        _, nz, ny, nx = planes.shape
        _lib.get_cast().call("scsfm_cast_cast", nx, ny, nz, *vol.origin, vol.voxel, _ptr(vol.planes), float(min_weight),
                             float(np.float32(near)), float(np.float32(step)), int(n_steps), V, H, W, _ptr(rec), _ptr(mk),
                             _ptr(depth), _ptr(normal), _ptr(rgb), _ptr(sh), _stream(vol.device))
        assert RC.same_bits(vol.planes.cpu().numpy(), planes)  # (the volume is only read)
        got = {}
        for key, t, count, shape in (("depth", depth, n, (V, H, W)), ("normal", normal, 3 * n, (V, 3, H, W)),
                                     ("rgb", rgb, 3 * n, (V, H, W, 3)), ("shade", sh, n, (V, H, W))):
            if t is None:
                got[key] = None
                continue
            tail = t[count:]
            assert bool(torch.isnan(tail).all() if t.dtype == torch.float32 else (tail == 0xAB).all()), f"{key}: guard"
            got[key] = t[:count].reshape(shape).cpu().numpy()
        return got


@pytest.mark.parametrize("name", RC.NAMES)
def test_case_equals_the_oracle_bit_for_bit(name):
    RC.check(name, Backend)


def test_views_in_batches():
    RC.check_batches(Backend)


def test_null_outputs():
    RC.check_null_outputs(Backend)


def test_views_equal_the_oracle():
    from scsfm_hip import raycast
    rng = np.random.default_rng(5)
    c2w = rng.standard_normal((5, 3, 4)) * np.array([1, 1, 1, 1e3])
    c2w[2, 1, 3], c2w[3, 0, 0] = 1e-320, np.pi
    got = raycast.views(torch.from_numpy(c2w).to(DEV), torch.from_numpy(RC.K).to(DEV)).cpu().numpy()
    assert RC.same_bits(got, RO.views(c2w, RC.K))


def test_python_layer_defaults_and_refusals():
    """Volume.raycast with its defaults (step = the voxel size, n_steps = ceil((far - near) / step), the cull) equals the
    oracle on the "plane" case, with cull=False too; CPU, float64, non-contiguous inputs and bad marches are refused"""
    from scsfm_hip import raycast
    case, ref = RC.cases()["plane"], RC.reference("plane")
    vol = _volume(case["planes"], case["origin"], case["voxel"])
    poses = [RC.pose(pos=(0.0, 0.0, 0.0)), RC.pose(0.25, -0.15, (0.3, 0.1, 0.2))]
    c2w = torch.from_numpy(np.stack(poses)).to(DEV)
    K = torch.from_numpy(RC.K).to(DEV)
    assert RC.same_bits(RO.views(np.stack(poses), RC.K), case["view"])
    far = float(np.float32(case["voxel"])) * case["n_steps"] - 1e-4     # ceil gives the case's 30 steps
    for kwargs in ({}, {"cull": False}, {"mask": raycast.brick_mask(vol, 1.0)}):
        got = vol.raycast(c2w, K, RC.HW, 0.0, far, **kwargs)
        assert isinstance(got, raycast.Cast) and got.depth.is_cuda
        RC.compare({k: getattr(got, k).cpu().numpy() for k in RC.KEYS}, ref, f"Volume.raycast {kwargs}")
    got = vol.raycast(c2w, K, RC.HW, 0.0, far, normals=False, colour=False, shade=False)
    assert got.normal is None and got.rgb is None and got.shade is None
    assert RC.same_bits(got.depth.cpu().numpy(), ref["depth"])
    with pytest.raises(TypeError, match="float64"):
        vol.raycast(c2w.float(), K, RC.HW, 0.0, far)
    with pytest.raises(TypeError, match="HIP device"):
        vol.raycast(c2w.cpu(), K, RC.HW, 0.0, far)
    with pytest.raises(TypeError, match="float32"):
        vol.raycast(c2w, K.double(), RC.HW, 0.0, far)
    with pytest.raises(ValueError, match="contiguous"):
        vol.raycast(c2w.transpose(1, 2), K, RC.HW, 0.0, far)
    with pytest.raises(ValueError, match="contiguous"):
        vol.raycast(c2w, K.t(), RC.HW, 0.0, far)
    with pytest.raises(TypeError, match="HIP device"):
        raycast.cast(type("V", (), dict(planes=vol.planes.cpu(), origin=vol.origin, voxel=vol.voxel))(), c2w, K, RC.HW, 0, far)
    for near, far_, step in ((0.0, 0.0, None), (-1.0, 1.0, None), (0.0, 1.0, 0.0), (0.0, 1.0, 1e-8), (0.0, float("nan"), None)):
        with pytest.raises(ValueError):
            vol.raycast(c2w, K, RC.HW, near, far_, step=step)
    with pytest.raises(ValueError, match="brick mask"):
        vol.raycast(c2w, K, RC.HW, 0.0, far, mask=torch.ones(7, dtype=torch.uint8, device=DEV))


def _files(folder):
    import os
    return sorted(os.listdir(str(folder)))


def test_reconstruct_render_on_six_generated_frames(tmp_path, capsys):
    """reconstruct.py --render on six generated 64 x 96 frames with randomly initialised nets saved by the test: the three
    older files are the same bytes as without the flag; fused_depth.npy is Volume.raycast on the tensors the hooks saw;
    the PNGs decode to the rgb and shade tensors; the printed agreement equals numpy's on those tensors to 1e-6; and
    --render-poses with the run's own poses.txt gives the oracle's cast of the re-read poses, bit for bit"""
    from PIL import Image

    import models
    import reconstruct
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
            "--frames-per-launch", "2", "--mesh"]
    plain, out, novel = tmp_path / "plain", tmp_path / "out", tmp_path / "novel"
    seen = {"batches": [], "renders": []}
    # (two runs of the nets give the same predictions only with MIOpen's reproducible solvers, as smoke() asks for them)
    old = torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = True, False
    try:
        reconstruct.main(argv + ["--output-dir", str(plain)])
        capsys.readouterr()
        vol = reconstruct.main(argv + ["--render", "--output-dir", str(out)],
                               on_batch=lambda *t: seen["batches"].append([x.clone() for x in t]),
                               on_render=lambda got, views: seen["renders"].append((got, views.clone())))
        printed = capsys.readouterr().out
        vol2 = reconstruct.main(argv + ["--render-poses", str(out / "poses.txt"), "--output-dir", str(novel)])
        printed_novel = capsys.readouterr().out
    finally:
        torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = old
    assert _files(plain) == ["mesh.ply", "poses.txt", "reconstruction.ply"]
    assert _files(out) == ["fused_depth.npy", "mesh.ply", "poses.txt", "reconstruction.ply", "render"]
    for name in ("mesh.ply", "poses.txt", "reconstruction.ply"):
        assert (plain / name).read_bytes() == (out / name).read_bytes(), name
    # fused_depth.npy is Volume.raycast on what the hooks saw
    disp, _, c2w = (torch.cat([b[k] for b in seen["batches"]]) for k in range(3))
    K = seen["batches"][0][3]
    assert len(seen["renders"]) == 2 and torch.equal(torch.cat([v for _, v in seen["renders"]]), c2w)
    fused = np.load(str(out / "fused_depth.npy"))
    assert fused.dtype == np.float32 and fused.shape == (6, 64, 96)
    far = 2.0 + vol.trunc
    want = vol.raycast(c2w, K, (64, 96), 0.0, far, min_weight=1.0)
    assert RC.same_bits(fused, want.depth.cpu().numpy())
    assert RC.same_bits(fused, torch.cat([g.depth for g, _ in seen["renders"]]).cpu().numpy())
    hit = fused > 0
    assert hit.any()
    print(f"share of pixels with a hit: {hit.mean():.4f}")
    # the pictures decode to the tensors
    assert _files(out / "render") == sorted(f"{k:06d}_{kind}.png" for k in range(6) for kind in ("colour", "shade"))
    rgb, shade = want.rgb.cpu().numpy(), want.shade.cpu().numpy()
    for k in range(6):
        assert np.array_equal(np.asarray(Image.open(str(out / "render" / f"{k:06d}_colour.png"))), rgb[k])
        assert np.array_equal(np.asarray(Image.open(str(out / "render" / f"{k:06d}_shade.png"))), shade[k])
    # the agreement line
    line = [ln for ln in printed.splitlines() if ln.startswith("rendered ")]
    assert len(line) == 1
    m = re.fullmatch(r"rendered 6 views -> \S+fused_depth\.npy: (\S+) of the pixels with a hit; mean \|pred - fused\| / fused "
                     r"(\S+) over (\d+) pixels", line[0])
    assert m, line[0]
    with np.errstate(all="ignore"):
        pred = np.float32(1) / disp[:, 0].cpu().numpy()
        both = hit & (pred <= np.float32(2.0))
        ratio = np.abs(pred.astype(np.float64) - fused.astype(np.float64)) / fused.astype(np.float64)
    assert float(m.group(1)) == pytest.approx(hit.mean(), rel=1e-6) and int(m.group(3)) == both.sum() > 0
    assert float(m.group(2)) == pytest.approx(ratio[both].mean(), rel=1e-6)
    # --render-poses with the run's own trajectory: the oracle's cast of the re-read poses, bit for bit
    assert torch.equal(vol2.planes, vol.planes)
    again = np.load(str(novel / "fused_depth.npy"))
    poses = np.loadtxt(str(out / "poses.txt")).reshape(-1, 3, 4)
    n_steps = int(np.ceil(far / vol.voxel))
    ref = RO.cast(vol2.planes.cpu().numpy(), vol2.origin, vol2.voxel, RO.views(poses, K.cpu().numpy()), (64, 96), 0.0, vol.voxel,
                  n_steps, 1.0)
    assert RC.same_bits(again, ref["depth"]) and ref["hit"].any()
    assert _files(novel / "render") == sorted(f"{k:06d}_{kind}.png" for k in range(6) for kind in ("colour", "shade"))
    assert np.array_equal(np.asarray(Image.open(str(novel / "render" / "000003_colour.png"))), ref["rgb"][3])
    assert np.array_equal(np.asarray(Image.open(str(novel / "render" / "000003_shade.png"))), ref["shade"][3])
    assert re.search(r"rendered 6 views -> \S+: \S+ of the pixels with a hit$", printed_novel, re.M)
    for name in ("mesh.ply", "poses.txt", "reconstruction.ply"):
        assert (plain / name).read_bytes() == (novel / name).read_bytes(), name
