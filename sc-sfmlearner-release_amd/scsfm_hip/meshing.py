"""A triangle mesh of the surface in a fused volume through libscsfm_mesh.so (include/scsfm_mesh.h): marching tetrahedra on
the voxel grid, with shared vertices, faces that index them, one orientation (counter-clockwise seen from free space) and
no cracks, bit-identical from run to run.

    vol = fusion.Volume(dims, origin, 0.05, device="cuda")
    vol.integrate(disp, images, c2w, K, is_disp=True, max_depth=10.0)
    xyz, rgb, tri = vol.extract_mesh(min_weight=2)          # or meshing.extract_mesh(vol, 2)
    write_ply_mesh("scene_mesh.ply", xyz, rgb, tri)

Everything stays on the device; extract_mesh() copies sixteen bytes (the two totals) to the host.  The vertices on the
grid's +x, +y and +z edges are, in order, the points of Volume.extract.  There is no torch fallback: without a HIP device
or the library this raises, and so do float64, CPU and non-contiguous tensors.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _lib

INT32_MAX = 2 ** 31 - 1


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream(device):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _planes(volume):
    """the five planes [5, nz, ny, nx] of a fusion.Volume (or the tensor itself), checked"""
    planes = getattr(volume, "planes", volume)
    if not isinstance(planes, torch.Tensor):
        raise TypeError(f"the volume's planes must be a torch tensor, got {type(planes).__name__}")
    if not planes.is_cuda:
        raise TypeError("the volume's planes must live on the HIP device (the mesh kernels have no CPU fallback)")
    if planes.dtype != torch.float32:
        raise TypeError(f"the volume's planes must be torch.float32, got {planes.dtype}")
    if not planes.is_contiguous():
        raise ValueError("the volume's planes must be contiguous")
    if planes.dim() != 4 or planes.shape[0] != 5:
        raise ValueError(f"the volume's planes must be [5, nz, ny, nx], got {list(planes.shape)}")
    return planes


def count(volume, min_weight=1.0):
    """-> (the number of vertices, the number of triangles, the workspace the writers need); sixteen bytes cross to the
    host"""
    planes = _planes(volume)
    _, nz, ny, nx = planes.shape
    lib = _lib.get_mesh()
    n = lib.size("scsfm_mesh_ws_bytes", nx, ny, nz)
    if not n:
        raise ValueError(f"a volume of {(nx, ny, nz)} voxels is refused: every size must be positive and their product "
                         f"at most 2^29")
    ws = torch.empty(n // 8, dtype=torch.int64, device=planes.device)
    lib.call("scsfm_mesh_count", nx, ny, nz, _ptr(planes), float(min_weight), _ptr(ws), n, _stream(planes.device))
    v, t = (int(k) for k in ws[:2].tolist())
    return v, t, ws


def _check_out(name, t, dtype, device):
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.device != device:
        raise TypeError(f"{name} must be a tensor on the volume's HIP device")
    if t.dtype != dtype:
        raise TypeError(f"{name} must be {dtype}, got {t.dtype}")
    if t.dim() != 2 or t.shape[1] != 3 or not t.is_contiguous():
        raise ValueError(f"{name} must be a contiguous [N, 3], got {list(t.shape)}")
    return t


def extract_mesh(volume, min_weight=1.0, vertex_capacity=None, triangle_capacity=None, out=None):
    """-> (xyz float32 [V, 3], rgb uint8 [V, 3], tri int32 [T, 3]) on the device, in the header's orders.  ``volume`` is
    a fusion.Volume.  With a capacity the arrays have that many rows and the items at and past it are dropped (rows past
    the count are left as allocated).  ``out`` = (xyz, rgb, tri) gives the arrays to write into instead; their rows are
    the capacities, and rows at and past the counts are left untouched."""
    planes = _planes(volume)
    _, nz, ny, nx = planes.shape
    origin, voxel = volume.origin, volume.voxel
    v, t, ws = count(volume, min_weight)
    if v > INT32_MAX or t > INT32_MAX:
        raise ValueError(f"{v} vertices and {t} triangles: a mesh whose indices pass int32 (2^31 - 1) is refused (choose "
                         f"a larger voxel size)")
    vcap = v if vertex_capacity is None else int(vertex_capacity)
    tcap = t if triangle_capacity is None else int(triangle_capacity)
    dev = planes.device
    if out is not None:
        xyz, rgb, tri = out
        _check_out("out[0] (xyz)", xyz, torch.float32, dev)
        _check_out("out[1] (rgb)", rgb, torch.uint8, dev)
        _check_out("out[2] (tri)", tri, torch.int32, dev)
        if len(rgb) != len(xyz):
            raise ValueError("out: xyz and rgb must have the same number of rows")
        vcap, tcap = len(xyz), len(tri)
    else:
        xyz = torch.empty((vcap, 3), dtype=torch.float32, device=dev)
        rgb = torch.empty((vcap, 3), dtype=torch.uint8, device=dev)
        tri = torch.empty((tcap, 3), dtype=torch.int32, device=dev)
    lib, stream, nbytes = _lib.get_mesh(), _stream(dev), ws.numel() * 8
    lib.call("scsfm_mesh_vertices", nx, ny, nz, *origin, voxel, _ptr(planes), float(min_weight), _ptr(ws), nbytes, v,
             vcap, _ptr(xyz) if vcap else None, _ptr(rgb) if vcap else None, stream)
    lib.call("scsfm_mesh_triangles", nx, ny, nz, _ptr(planes), float(min_weight), _ptr(ws), nbytes, v, t, tcap,
             _ptr(tri) if tcap else None, stream)
    return xyz, rgb, tri


def write_ply_mesh(path, xyz, rgb, tri):
    """A binary little-endian PLY: the vertices as fusion.write_ply writes them (float x y z, uchar red green blue), then
    the faces as a list of three int vertex indices each."""
    host = lambda a: a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)  # noqa: E731
    xyz, rgb, tri = host(xyz), host(rgb), host(tri)
    if xyz.ndim != 2 or xyz.shape[1] != 3 or rgb.shape != xyz.shape:
        raise ValueError(f"xyz and rgb must both be [V, 3], got {list(xyz.shape)} and {list(rgb.shape)}")
    if tri.ndim != 2 or tri.shape[1] != 3:
        raise ValueError(f"tri must be [T, 3], got {list(tri.shape)}")
    if xyz.dtype.kind != "f" or rgb.dtype != np.uint8 or tri.dtype.kind not in "iu":
        raise TypeError(f"xyz must be floating point, rgb uint8 and tri an integer type, got {xyz.dtype}, {rgb.dtype} "
                        f"and {tri.dtype}")
    if len(tri) and (int(tri.min()) < 0 or int(tri.max()) >= len(xyz)):
        raise ValueError(f"tri must index the {len(xyz)} vertices")
    verts = np.empty(len(xyz), dtype=[("xyz", "<f4", 3), ("rgb", "u1", 3)])
    verts["xyz"], verts["rgb"] = xyz, rgb
    faces = np.empty(len(tri), dtype=[("n", "u1"), ("idx", "<i4", 3)])
    faces["n"], faces["idx"] = 3, tri
    header = ("ply\nformat binary_little_endian 1.0\nelement vertex {}\nproperty float x\nproperty float y\n"
              "property float z\nproperty uchar red\nproperty uchar green\nproperty uchar blue\nelement face {}\n"
              "property list uchar int vertex_indices\nend_header\n")
    with open(path, "wb") as f:
        f.write(header.format(len(xyz), len(tri)).encode("ascii"))
        f.write(verts.tobytes())
        f.write(faces.tobytes())
