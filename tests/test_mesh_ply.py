"""scsfm_hip.meshing.write_ply_mesh on a two-triangle mesh: the header's text and the file's length are exact, the faces
parse back, an empty mesh is handled, and shape and dtype mistakes are refused."""
import numpy as np
import pytest
import torch

from scsfm_hip import meshing

XYZ = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0.5], [0, 1, -2.25]], np.float32)
RGB = np.array([[0, 1, 2], [255, 254, 253], [10, 20, 30], [7, 7, 7]], np.uint8)
TRI = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
HEADER = ("ply\nformat binary_little_endian 1.0\nelement vertex {}\nproperty float x\nproperty float y\nproperty float z\n"
          "property uchar red\nproperty uchar green\nproperty uchar blue\nelement face {}\n"
          "property list uchar int vertex_indices\nend_header\n")


def _parse(blob, nv, nf):
    head = HEADER.format(nv, nf).encode("ascii")
    assert blob.startswith(head) and len(blob) == len(head) + 15 * nv + 13 * nf
    body = blob[len(head):]
    verts = np.frombuffer(body[:15 * nv], dtype=[("xyz", "<f4", 3), ("rgb", "u1", 3)])
    faces = np.frombuffer(body[15 * nv:], dtype=[("n", "u1"), ("idx", "<i4", 3)])
    return verts, faces


@pytest.mark.parametrize("as_tensor", [False, True])
def test_two_triangles(tmp_path, as_tensor):
    path = str(tmp_path / "mesh.ply")
    args = [torch.from_numpy(a) for a in (XYZ, RGB, TRI)] if as_tensor else [XYZ, RGB, TRI]
    meshing.write_ply_mesh(path, *args)
    verts, faces = _parse(open(path, "rb").read(), 4, 2)
    assert np.array_equal(verts["xyz"], XYZ) and np.array_equal(verts["rgb"], RGB)
    assert faces["n"].tolist() == [3, 3] and np.array_equal(faces["idx"], TRI)


def test_the_vertices_are_what_write_ply_writes(tmp_path):
    from scsfm_hip import fusion
    a, b = str(tmp_path / "a.ply"), str(tmp_path / "b.ply")
    fusion.write_ply(a, XYZ, RGB)
    meshing.write_ply_mesh(b, XYZ, RGB, TRI)
    points = open(a, "rb").read().split(b"end_header\n", 1)[1]
    assert open(b, "rb").read().split(b"end_header\n", 1)[1][:len(points)] == points and len(points) == 60


def test_an_empty_mesh(tmp_path):
    path = str(tmp_path / "empty.ply")
    meshing.write_ply_mesh(path, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.uint8), np.zeros((0, 3), np.int32))
    assert open(path, "rb").read() == HEADER.format(0, 0).encode("ascii")
    meshing.write_ply_mesh(path, XYZ, RGB, np.zeros((0, 3), np.int32))  # (vertices without a face)
    _parse(open(path, "rb").read(), 4, 0)


def test_mistakes_are_refused(tmp_path):
    path = str(tmp_path / "bad.ply")
    for xyz, rgb, tri, error in ((XYZ[:, :2], RGB, TRI, ValueError), (XYZ, RGB[:3], TRI, ValueError),
                                 (XYZ, RGB, TRI[:, :2], ValueError), (XYZ, RGB, TRI.reshape(-1), ValueError),
                                 (XYZ, RGB.astype(np.float32), TRI, TypeError), (XYZ, RGB, TRI.astype(np.float32), TypeError),
                                 (XYZ.astype(np.int32), RGB, TRI, TypeError), (XYZ, RGB, TRI + 2, ValueError),
                                 (XYZ, RGB, TRI - 1, ValueError)):
        with pytest.raises(error):
            meshing.write_ply_mesh(path, xyz, rgb, tri)
    assert not (tmp_path / "bad.ply").exists()
