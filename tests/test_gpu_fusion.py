"""scsfm_hip.fusion (libscsfm_fuse.so) on the device against tests/fusion_oracle.py, bit for bit: the cases of
tests/_fusion_cases.py, which tests/test_fusion_hostsim.py runs on the host simulator; then what only the device shows --
Volume.integrate split into launches, the refusals of the Python layer, and reconstruct.py end to end."""
import numpy as np
import pytest
import torch

import _fusion_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda"


class Backend:
    @staticmethod
    def volume(dims, origin, voxel, trunc, max_weight, frames_per_launch):
        from scsfm_hip import fusion
        return fusion.Volume(dims, origin, voxel, trunc, max_weight, DEV, frames_per_launch)

    @staticmethod
    def set_planes(vol, planes):
        vol.planes.copy_(torch.from_numpy(planes))

    dev = staticmethod(lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV))
    host = staticmethod(lambda t: t.cpu().numpy())

    @staticmethod
    def extract_guarded(vol, min_weight, capacity):
        """the library's call into buffers with 64 rows of fill behind the capacity, which must stay as they are"""
        from scsfm_hip.fusion import _ptr, _stream
        _, ws = vol.count(min_weight)
        xyz = torch.full((capacity + 64, 3), float("nan"), device=DEV)
        rgb = torch.full((capacity + 64, 3), 0xAB, dtype=torch.uint8, device=DEV)
        vol._lib.call("scsfm_fuse_extract", *vol.dims, *vol.origin, vol.voxel, _ptr(vol.planes), float(min_weight),
                      _ptr(ws), ws.numel() * 4, capacity, _ptr(xyz), _ptr(rgb), _stream(vol.device))
        assert bool(torch.isnan(xyz[capacity:]).all()) and bool((rgb[capacity:] == 0xAB).all())
        return xyz[:capacity].cpu().numpy(), rgb[:capacity].cpu().numpy()


@pytest.mark.parametrize("name", C.NAMES)
def test_case_equals_the_oracle_bit_for_bit(name):
    _, n = C.check(name, Backend)
    assert (n == 0) == (name == "empty")


def test_capacity_below_and_at_the_count():
    C.check_capacity("straddle_F5", Backend)


def test_cameras_equal_the_oracle():
    import fusion_oracle as O
    from scsfm_hip import fusion
    case = C.cases()["straddle_F8_vec"]["calls"][0]
    got = fusion.cameras(Backend.dev(case["c2w"]), Backend.dev(C.K)).cpu().numpy()
    assert C.same_bits(got, O.cameras(case["c2w"], C.K))


def test_analytic_plane():
    """A fronto-parallel plane at depth D0 = 1.73 seen by three cameras with identity rotation: every point on a z-edge
    lies within four times the oracle's own largest deviation from D0, and at least 90 % of the in-frustum columns yield
    a point.

    Measured on an MI355X: largest |z - D0| 1.907e-08 for the oracle and for the device (every z is the float nearest to
    1.73), every in-frustum column (100 %) with a point for both.  The test prints the figures."""
    from scsfm_hip import fusion
    ref, xyz, _, axis = C.analytic_reference()
    dev_ref, share_ref = C.plane_statistics(xyz, axis)
    vol = fusion.Volume(**C.ANALYTIC, device=DEV)
    call = C.analytic_call()
    vol.integrate(Backend.dev(call["depth"]), None, Backend.dev(call["c2w"]), Backend.dev(call["K"]), is_disp=False,
                  near=call["near"], max_depth=call["max_depth"])
    got_xyz = vol.extract(1.0)[0].cpu().numpy()
    assert len(got_xyz) == len(xyz)
    dev, share = C.plane_statistics(got_xyz, axis)
    print(f"oracle: largest |z - D0| {dev_ref:.3e}, share {share_ref:.3f}; device: {dev:.3e}, share {share:.3f}")
    assert dev <= 4 * dev_ref and share >= 0.9 and share_ref >= 0.9
    assert C.same_bits(got_xyz, xyz) and C.same_bits(vol.planes.cpu().numpy(), ref.planes)


def test_integrate_split_into_launches_equals_one_launch():
    """40 frames (the case's eight, five times over): frames_per_launch 40 -- two launches inside the library, which
    carries 32 a launch --, 8, 3 and 1 leave the same bits"""
    call = C.cases()["straddle_F8_vec"]["calls"][0]
    args = [Backend.dev(np.concatenate([call[k]] * 5)) for k in ("depth", "images", "c2w")] + [Backend.dev(C.K)]
    planes = []
    for fpl in (40, 8, 3, 1):
        vol = Backend.volume((40, 18, 29), C.ORIGIN, C.VOXEL, None, 16.0, fpl)
        vol.integrate(*args, is_disp=False, near=0.05, max_depth=4.0)
        planes.append(vol.planes)
    assert float(planes[0][1].max()) == 16.0
    assert all(torch.equal(planes[0], p) for p in planes[1:])


def test_refusals():
    from scsfm_hip import fusion
    vol = fusion.Volume((8, 6, 5), (0, 0, 0), 0.1, device=DEV)
    d, img = torch.ones((2, 12, 20), device=DEV), torch.zeros((2, 3, 12, 20), device=DEV)
    c2w = Backend.dev(np.stack([C.pose(), C.pose()]))
    K = Backend.dev(C.K)
    vol.integrate(d, img, c2w, K)
    with pytest.raises(TypeError, match="float32"):
        vol.integrate(d.double(), img, c2w, K)
    with pytest.raises(TypeError, match="float64"):
        vol.integrate(d, img, c2w.float(), K)
    with pytest.raises(TypeError, match="HIP device"):
        vol.integrate(d.cpu(), img, c2w, K)
    with pytest.raises(ValueError, match="contiguous"):
        vol.integrate(d.transpose(1, 2), img, c2w, K)
    with pytest.raises(ValueError, match="contiguous"):
        vol.integrate(d, img[:, :, :, ::2], c2w, K)
    with pytest.raises(ValueError):
        vol.integrate(d, img[:1].contiguous(), c2w, K)
    with pytest.raises(ValueError, match="2\\^29"):
        fusion.Volume((1024, 1024, 513), (0, 0, 0), 0.1, device=DEV)
    with pytest.raises(_lib_error()):
        vol.extract(min_weight=0.5)


def _lib_error():
    from scsfm_hip._lib import ScsfmError
    return ScsfmError


def _read_ply(path):
    blob = open(path, "rb").read()
    head, body = blob.split(b"end_header\n", 1)
    lines = head.decode("ascii").splitlines()
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0"
    n = int([ln for ln in lines if ln.startswith("element vertex")][0].split()[-1])
    assert [ln for ln in lines if ln.startswith("property")] == [
        "property float x", "property float y", "property float z", "property uchar red", "property uchar green",
        "property uchar blue"]
    rec = np.frombuffer(body, dtype=[("xyz", "<f4", 3), ("rgb", "u1", 3)])
    assert len(rec) == n
    return rec["xyz"], rec["rgb"]


def test_reconstruct_on_six_generated_frames(tmp_path):
    """reconstruct.py on six generated 64 x 96 frames with randomly initialised nets saved by the test: the PLY parses,
    holds what Volume.extract gives on the same inputs in one launch, poses.txt is chain_poses' trajectory, and a volume
    above 2^29 voxels is refused"""
    from PIL import Image

    import models
    import reconstruct
    from scsfm_hip import fusion
    from scsfm_hip.odometry import chain_poses
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
    seen = {"batches": []}
    out = tmp_path / "out"
    argv = ["--pretrained-dispnet", str(tmp_path / "disp.pth.tar"), "--pretrained-posenet", str(tmp_path / "pose.pth.tar"),
            "--dataset-dir", str(frames), "--intrinsics", str(tmp_path / "cam.txt"), "--img-height", "64", "--img-width",
            "96", "--batch-size", "4", "--max-depth", "2.0", "--resolution", "96", "--min-weight", "1",
            "--frames-per-launch", "2", "--output-dir", str(out)]
    vol = reconstruct.main(argv, on_poses=lambda v: seen.update(vec=v.clone()),
                           on_batch=lambda *t: seen["batches"].append([x.clone() for x in t]))
    xyz, rgb = _read_ply(str(out / "reconstruction.ply"))
    assert len(seen["batches"]) == 2 and seen["vec"].shape == (5, 6)
    disp, imgs, c2w = (torch.cat([b[k] for b in seen["batches"]]) for k in range(3))
    K = seen["batches"][0][3]
    assert disp.shape == (6, 1, 64, 96) and K.cpu().numpy().tolist() == [[58.0, 0, 47.5], [0, 58.0, 31.5], [0, 0, 1]]
    mine = fusion.Volume(vol.dims, vol.origin, vol.voxel, vol.trunc, device=DEV, frames_per_launch=6)
    mine.integrate(disp, imgs, c2w, K, is_disp=True, max_depth=2.0)
    want_xyz, want_rgb = mine.extract(1.0)
    assert max(vol.dims) == 96 and len(xyz) == len(want_xyz) and len(xyz) > 0
    assert C.same_bits(xyz, want_xyz.cpu().numpy()) and C.same_bits(rgb, want_rgb.cpu().numpy())
    poses = chain_poses(seen["vec"]).reshape(-1, 12)
    assert torch.equal(poses, c2w.reshape(-1, 12))
    text = np.loadtxt(str(out / "poses.txt"))
    want = np.array([[float("%1.8e" % v) for v in row] for row in poses.cpu().numpy()])
    assert text.shape == (6, 12) and np.array_equal(text, want) and np.array_equal(text[0], np.eye(4)[:3].reshape(-1))
    # a voxel size that would need more than 2^29 voxels is refused, by the flag's name, before anything is allocated
    with pytest.raises(SystemExit, match="--voxel-size"):
        reconstruct.main(argv[:argv.index("--resolution")] + ["--voxel-size", "0.004", "--output-dir", str(out)])
