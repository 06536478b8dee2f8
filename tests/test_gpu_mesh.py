"""scsfm_hip.meshing (libscsfm_mesh.so) on the device against tests/mesh_oracle.py, bit for bit: the cases of
tests/_fusion_cases.py fused on the device and the volumes of tests/_mesh_cases.py, which tests/test_mesh_hostsim.py runs on
the host simulator; then what only the device shows -- the Python layer's refusals and reconstruct.py --mesh end to end."""
import numpy as np
import pytest
import torch

import _fusion_cases as FC
import _mesh_cases as MC
import mesh_oracle as MO

pytestmark = pytest.mark.gpu
DEV = "cuda"


class Backend:
    """what tests/_fusion_cases.run needs to fuse a case on the device"""

    @staticmethod
    def volume(dims, origin, voxel, trunc, max_weight, frames_per_launch):
        from scsfm_hip import fusion
        return fusion.Volume(dims, origin, voxel, trunc, max_weight, DEV, frames_per_launch)

    @staticmethod
    def set_planes(vol, planes):
        vol.planes.copy_(torch.from_numpy(planes))

    dev = staticmethod(lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV))


def _volume(planes, origin, voxel):
    from scsfm_hip import fusion
    _, nz, ny, nx = planes.shape
    vol = fusion.Volume((nx, ny, nz), origin, voxel, device=DEV)
    vol.planes.copy_(torch.from_numpy(np.array(planes)))  # (a writable copy)
    return vol


def _host(arrays):
    return tuple(a.cpu().numpy() for a in arrays)


def _mesh(planes, origin, voxel, min_weight, vcap=None, tcap=None):
    """meshing.extract_mesh into buffers filled with NaN / 0xAB, 64 rows longer than the capacity: those stay as they are"""
    from scsfm_hip import meshing
    vol = _volume(planes, origin, voxel)
    if vcap is None and tcap is None:
        return _host(vol.extract_mesh(min_weight))
    xyz = torch.full((vcap + 64, 3), float("nan"), device=DEV)
    rgb = torch.full((vcap + 64, 3), 0xAB, dtype=torch.uint8, device=DEV)
    tri = torch.full((tcap + 64, 3), 0xAB, dtype=torch.int32, device=DEV)
    meshing.extract_mesh(vol, min_weight, out=(xyz[:vcap], rgb[:vcap], tri[:tcap]))
    assert bool(torch.isnan(xyz[vcap:]).all()) and bool((rgb[vcap:] == 0xAB).all()) and bool((tri[tcap:] == 0xAB).all())
    return _host((xyz[:vcap], rgb[:vcap], tri[:tcap]))


@pytest.mark.parametrize("name", FC.NAMES)
def test_fusion_cases_equal_the_oracle(name):
    case = FC.cases()[name]
    vol = FC.run(case, Backend, 8)
    planes = FC.reference(name)[0].planes
    assert MC.same_bits(vol.planes.cpu().numpy(), planes)
    for min_weight in (1.0, 2.0):
        ref = MO.mesh(planes, vol.origin, vol.voxel, min_weight)
        xyz, rgb, tri = _host(vol.extract_mesh(min_weight))
        MC.check_against(ref, xyz, rgb, tri, f"{name} at min_weight {min_weight}")
        pts, cols = _host(vol.extract(min_weight))
        axial = ref["e"] < 3
        assert MC.same_bits(xyz[axial], pts) and MC.same_bits(rgb[axial], cols), name


def test_planes_filled_by_hand_equal_the_oracle():
    for min_weight in (MC.DIRECT_MIN_WEIGHT, 1.0, 3.0):
        ref = MC.direct_reference(min_weight)
        got = _mesh(MC.direct_planes(), MC.DIRECT_ORIGIN, MC.DIRECT_VOXEL, min_weight)
        MC.check_against(ref, *got, f"min_weight {min_weight}")


@pytest.mark.parametrize("dims", [(1, 6, 5), (6, 1, 5), (6, 5, 1)])
def test_a_volume_one_voxel_thick_has_no_triangle(dims):
    nx, ny, nz = dims
    rng = np.random.default_rng(5)
    planes = np.zeros((5, nz, ny, nx), np.float32)
    planes[0] = rng.uniform(-1, 1, (nz, ny, nx))
    planes[1] = rng.integers(0, 3, (nz, ny, nx))
    ref = MO.mesh(planes, (0.0, 0.5, -0.5), 0.25, 1.0)
    xyz, rgb, tri = _mesh(planes, (0.0, 0.5, -0.5), 0.25, 1.0)
    assert len(xyz) > 0 and tri.shape == (0, 3)
    MC.check_against(ref, xyz, rgb, tri, str(dims))


def test_nothing_is_written_at_or_past_the_capacity():
    MC.check_capacity(_mesh, None, None, None)  # (_mesh itself checks the fill behind every capacity)


def test_the_sphere_is_a_closed_oriented_manifold():
    xyz, rgb, tri = _mesh(MC.sphere_planes(), (0.0, 0.0, 0.0), MC.SPHERE_VOXEL, 1.0)
    err, bound = MC.check_sphere(xyz, tri)  # (the device's own output)
    print(f"sphere: {len(xyz)} vertices, {len(tri)} triangles, largest distance to the sphere {err:.3e} (bound {bound:.3e})")
    MC.check_against(MC.sphere_reference(), xyz, rgb, tri, "sphere")


def test_two_extractions_give_equal_bytes():
    vol = FC.run(FC.cases()["straddle_F5"], Backend, 8)
    first, second = _host(vol.extract_mesh(1.0)), _host(vol.extract_mesh(1.0))
    assert all(MC.same_bits(a, b) for a, b in zip(first, second)) and len(first[2]) > 100


def test_refusals():
    from scsfm_hip import fusion, meshing
    from scsfm_hip._lib import ScsfmError
    vol = _volume(MC.direct_planes(), MC.DIRECT_ORIGIN, MC.DIRECT_VOXEL)

    class Host:
        origin, voxel = vol.origin, vol.voxel
        planes = vol.planes.cpu()
    with pytest.raises(TypeError, match="HIP device"):
        meshing.extract_mesh(Host)

    class Double(Host):
        planes = vol.planes.double()
    with pytest.raises(TypeError, match="float32"):
        meshing.extract_mesh(Double)

    class Strided(Host):
        planes = vol.planes[:, :, :, ::2]
    with pytest.raises(ValueError, match="contiguous"):
        meshing.extract_mesh(Strided)
    with pytest.raises(ScsfmError):
        vol.extract_mesh(min_weight=0.5)
    good = (torch.empty((4, 3), device=DEV), torch.empty((4, 3), dtype=torch.uint8, device=DEV),
            torch.empty((4, 3), dtype=torch.int32, device=DEV))
    with pytest.raises(TypeError, match="int32"):
        meshing.extract_mesh(vol, out=(good[0], good[1], good[2].long()))
    with pytest.raises(TypeError, match="HIP device"):
        meshing.extract_mesh(vol, out=(good[0].cpu(), good[1], good[2]))
    assert isinstance(vol, fusion.Volume)


def _read_ply_mesh(path):
    blob = open(path, "rb").read()
    head, body = blob.split(b"end_header\n", 1)
    lines = head.decode("ascii").splitlines()
    assert lines[:2] == ["ply", "format binary_little_endian 1.0"]
    nv, nf = int(lines[2].split()[-1]), int(lines[9].split()[-1])
    assert lines[2].startswith("element vertex ") and lines[9].startswith("element face ")
    assert lines[10] == "property list uchar int vertex_indices" and len(lines) == 11
    verts = np.frombuffer(body[:15 * nv], dtype=[("xyz", "<f4", 3), ("rgb", "u1", 3)])
    faces = np.frombuffer(body[15 * nv:], dtype=[("n", "u1"), ("idx", "<i4", 3)])
    assert len(faces) == nf and (faces["n"] == 3).all()
    return verts["xyz"], verts["rgb"], faces["idx"]


def test_reconstruct_with_and_without_mesh(tmp_path, capsys):
    """reconstruct.py on the six generated frames of tests/test_gpu_fusion.py, with and without --mesh: mesh.ply parses
    and holds Volume.extract_mesh of the returned volume; reconstruction.ply and poses.txt are the same bytes in the two
    runs; without the flag there is no mesh.ply and no line about one"""
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
            "--frames-per-launch", "2", "--output-dir"]
    plain, meshed = tmp_path / "plain", tmp_path / "meshed"
    # (two runs of the nets give the same predictions only with MIOpen's reproducible solvers, as smoke() asks for them)
    old = torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = True, False
    try:
        reconstruct.main(argv + [str(plain)])
        out_plain = capsys.readouterr().out
        vol = reconstruct.main(argv + [str(meshed), "--mesh"])
        out_meshed = capsys.readouterr().out
    finally:
        torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = old
    assert not (plain / "mesh.ply").exists() and "triangles" not in out_plain
    for name in ("reconstruction.ply", "poses.txt"):
        assert (plain / name).read_bytes() == (meshed / name).read_bytes(), name
    xyz, rgb, tri = _read_ply_mesh(str(meshed / "mesh.ply"))
    want = _host(vol.extract_mesh(1.0))
    assert len(tri) > 0 and all(MC.same_bits(a, b) for a, b in zip((xyz, rgb, tri), want))
    assert out_meshed.replace(str(meshed), "X") == out_plain.replace(str(plain), "X") + \
        "{} vertices, {} triangles -> {}\n".format(len(xyz), len(tri), "X/mesh.ply")
