"""Dense voxel reconstruction from predicted depth and poses through libscsfm_fuse.so (include/scsfm_fuse.h): a
truncated signed distance volume that frames are integrated into on the device, and the surface points read off it.

    origin, dims = bounds_from_cameras(c2w, 10.0, 0.05)
    vol = Volume(dims, origin, 0.05, device="cuda")
    vol.integrate(disp, images, c2w, K, is_disp=True, max_depth=10.0)     # any number of frames, in launches of
    xyz, rgb = vol.extract(min_weight=2)                                  # vol.frames_per_launch
    write_ply("scene.ply", xyz, rgb)

``disp`` is the disparity net's output [F, 1, H, W] (or [F, H, W]) and ``images`` its normalised input [F, 3, H, W]
(or None: geometry only); ``c2w`` is what scsfm_hip.odometry.chain_poses returns, float64 [F, 3, 4].  Everything stays on
the device; extract() copies one int (the number of points) to the host.  There is no torch fallback: without a HIP
device or the library this raises, and so do float64, CPU and non-contiguous tensors.
"""
from __future__ import annotations

import ctypes
import math

import numpy as np
import torch

from . import _lib

MAX_VOXELS = 1 << 29
# Frames a launch of the integration carries.  A voxel is read and written once per launch, so the volume's traffic falls
# as 1 / frames_per_launch while the registers stay the same.  Measured (tools/bench_fusion.py, profiles/fusion_bench.json:
# a 512 x 128 x 512 volume, 64 frames of 256 x 832, medians of 15): where every frame covers the volume, 0.339 ms a frame
# at 1, 0.159 at 4, 0.133 at 8 and 0.127 at 16 frames a launch; where a frame meets a seventh of the tiles, 0.086, 0.053,
# 0.050 and 0.050.  8 takes all but 4 % of what there is to take and asks the caller to hold 8 frames, not 16.
FRAMES_PER_LAUNCH = 8
TRUNC_VOXELS = 3.0  # the default truncation distance, in voxels


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _check(name, t, dtype, shape=None):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch tensor, got {type(t).__name__}")
    if not t.is_cuda:
        raise TypeError(f"{name} must live on the HIP device (the fusion kernels have no CPU fallback)")
    if t.dtype != dtype:
        raise TypeError(f"{name} must be {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name} must be {list(shape)}, got {list(t.shape)}")
    return t


def _stream(device):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def cameras(c2w, K):
    """c2w float64 [F, 3, 4] (or [F, 12]) and K float32 [3, 3] on the device -> the kernels' camera records, float32
    [F, 16]: world-to-camera rotation (9), translation (3), fx, fy, cx, cy."""
    _check("c2w", c2w, torch.float64)
    if c2w.numel() % 12 or c2w.shape[-1] not in (4, 12):
        raise ValueError(f"c2w must be [F, 3, 4] or [F, 12], got {list(c2w.shape)}")
    _check("K", K, torch.float32, (3, 3))
    n = c2w.numel() // 12
    cam = torch.empty((n, 16), dtype=torch.float32, device=c2w.device)
    if n:
        _lib.get_fuse().call("scsfm_fuse_cameras", n, _ptr(c2w), _ptr(K), _ptr(cam), _stream(c2w.device))
    return cam


class Volume:
    """A truncated signed distance volume of dims = (nx, ny, nz) voxels of ``voxel_size`` whose corner is ``origin``;
    ``trunc`` defaults to TRUNC_VOXELS voxels; a voxel's weight stops growing at ``max_weight``."""

    def __init__(self, dims, origin, voxel_size, trunc=None, max_weight=64.0, device="cuda",
                 frames_per_launch=FRAMES_PER_LAUNCH):
        if not torch.cuda.is_available():
            raise RuntimeError("the fusion kernels need a HIP device (there is no CPU fallback)")
        self.dims = tuple(int(d) for d in dims)
        self.origin = tuple(float(np.float32(o)) for o in origin)
        self.voxel = float(np.float32(voxel_size))
        self.trunc = float(np.float32(TRUNC_VOXELS * voxel_size if trunc is None else trunc))
        self.max_weight = float(max_weight)
        self.frames_per_launch = int(frames_per_launch)
        self.device = torch.device(device)
        if len(self.dims) != 3 or len(self.origin) != 3:
            raise ValueError("dims and origin must have three entries")
        if self.frames_per_launch < 1:
            raise ValueError("frames_per_launch must be at least 1")
        self._lib = _lib.get_fuse()
        nbytes = self._lib.size("scsfm_fuse_volume_bytes", *self.dims)
        if not nbytes:
            raise ValueError(f"a volume of {self.dims} voxels is refused: every size must be positive and their product "
                             f"at most 2^29 (choose a larger voxel size)")
        nx, ny, nz = self.dims
        self.planes = torch.zeros((5, nz, ny, nx), dtype=torch.float32, device=self.device)
        assert self.planes.numel() * 4 == nbytes

    @property
    def nbytes(self):
        return self.planes.numel() * 4

    @property
    def tsdf(self):
        return self.planes[0]

    @property
    def weight(self):
        return self.planes[1]

    @property
    def colour(self):
        return self.planes[2:]

    def integrate(self, disp_or_depth, images, c2w, K, is_disp=True, near=0.0, max_depth=10.0, weight=None):
        """Integrates F frames, in launches of ``frames_per_launch``: the nets' disparity (``is_disp``) or a depth
        [F, 1, H, W] / [F, H, W], the normalised images [F, 3, H, W] or None, the camera-to-world poses float64
        [F, 3, 4] and the intrinsics float32 [3, 3] of these H x W frames.  With ``weight`` (float32 [F, H, W], what
        scsfm_hip.confidence.weights gives) every observation counts by its pixel's weight instead of 1
        (scsfm_hip.confidence.integrate, libscsfm_conf.so)."""
        if weight is not None:
            from . import confidence
            return confidence.integrate(self, disp_or_depth, images, c2w, K, weight, is_disp=is_disp, near=near,
                                        max_depth=max_depth)
        d = _check("disp_or_depth", disp_or_depth, torch.float32)
        if d.dim() == 4 and d.shape[1] == 1:
            d = d[:, 0]
        if d.dim() != 3:
            raise ValueError(f"disp_or_depth must be [F, 1, H, W] or [F, H, W], got {list(disp_or_depth.shape)}")
        F, H, W = d.shape
        if images is not None:
            _check("images", images, torch.float32, (F, 3, H, W))
        cam = cameras(c2w, K)
        if cam.shape[0] != F:
            raise ValueError(f"{cam.shape[0]} poses for {F} frames")
        stream = _stream(self.device)
        for f0 in range(0, F, self.frames_per_launch):
            n = min(F, f0 + self.frames_per_launch) - f0
            self._lib.call("scsfm_fuse_integrate", *self.dims, *self.origin, self.voxel, self.trunc, float(near),
                           float(max_depth), self.max_weight, n, H, W, _ptr(cam[f0:]), _ptr(d[f0:]), int(bool(is_disp)),
                           None if images is None else _ptr(images[f0:]), _ptr(self.planes), stream)

    def count(self, min_weight=1.0):
        """-> (the number of surface points, the workspace extract() needs); one int crosses to the host"""
        n = self._lib.size("scsfm_fuse_extract_ws_bytes", *self.dims)
        ws = torch.empty(n // 4, dtype=torch.int32, device=self.device)
        self._lib.call("scsfm_fuse_count", *self.dims, _ptr(self.planes), float(min_weight), _ptr(ws), n,
                       _stream(self.device))
        return int(ws[0].item()), ws

    def extract(self, min_weight=1.0, capacity=None):
        """-> (xyz float32 [N, 3], rgb uint8 [N, 3]) on the device, in the header's order.  With ``capacity`` the two
        have that many rows and the points at and past it are dropped (rows past the count are left as allocated)."""
        total, ws = self.count(min_weight)
        cap = total if capacity is None else int(capacity)
        xyz = torch.empty((cap, 3), dtype=torch.float32, device=self.device)
        rgb = torch.empty((cap, 3), dtype=torch.uint8, device=self.device)
        self._lib.call("scsfm_fuse_extract", *self.dims, *self.origin, self.voxel, _ptr(self.planes), float(min_weight),
                       _ptr(ws), ws.numel() * 4, cap, _ptr(xyz) if cap else None, _ptr(rgb) if cap else None,
                       _stream(self.device))
        return xyz, rgb

    def extract_mesh(self, min_weight=1.0):
        """-> (xyz float32 [V, 3], rgb uint8 [V, 3], tri int32 [T, 3]) on the device: the surface as an indexed triangle
        mesh (scsfm_hip.meshing.extract_mesh, libscsfm_mesh.so)."""
        from . import meshing
        return meshing.extract_mesh(self, min_weight)

    def raycast(self, c2w, K, hw, near, far, **kwargs):
        """-> raycast.Cast(depth float32 [V, H, W], normal float32 [V, 3, H, W], rgb uint8 [V, H, W, 3], shade uint8
        [V, H, W]) on the device: the volume seen from the poses ``c2w`` (scsfm_hip.raycast.cast, libscsfm_cast.so)."""
        from . import raycast
        return raycast.cast(self, c2w, K, hw, near, far, **kwargs)

    def track(self, depth_or_disp, guess, K, **kwargs):
        """-> tracking.Track(c2w float64 [V, 3, 4], report, model_depth, model_normal, state) on the device: the poses
        ``guess`` of V frames refined against this volume by point-to-plane ICP (scsfm_hip.tracking.track,
        libscsfm_track.so)."""
        from . import tracking
        return tracking.track(self, depth_or_disp, guess, K, **kwargs)

    def track_scaled(self, depth_or_disp, guess, scale0, K, **kwargs):
        """-> similarity.Track(c2w float64 [V, 3, 4], scale float64 [V], report, model_depth, model_normal, state) on the
        device: the poses ``guess`` and the depth scales ``scale0`` of V frames refined against this volume by
        point-to-plane ICP over seven degrees of freedom (scsfm_hip.similarity.track, libscsfm_sim3.so)."""
        from . import similarity
        return similarity.track(self, depth_or_disp, guess, scale0, K, **kwargs)


def camera_box(c2w, max_depth):
    """The box of the camera centres grown by ``max_depth`` on every side -> (lo, hi), two float64 arrays of 3.
    c2w: [F, 3, 4] or [F, 12], a tensor or an array."""
    p = c2w.detach().cpu().numpy() if isinstance(c2w, torch.Tensor) else np.asarray(c2w)
    centres = p.reshape(-1, 3, 4)[:, :, 3].astype(np.float64)
    if not len(centres) or not np.isfinite(centres).all():
        raise ValueError("the box of the cameras needs at least one pose, all finite")
    if not max_depth > 0:
        raise ValueError("max_depth must be positive")
    return centres.min(axis=0) - max_depth, centres.max(axis=0) + max_depth


def bounds_from_cameras(c2w, max_depth, voxel_size):
    """camera_box in voxels of ``voxel_size`` -> (origin (3 floats), dims (3 ints)).  Dims are rounded up, so the box is
    covered (a side that is a whole number of voxels, to 1e-9 of a voxel, gets exactly that many)."""
    lo, hi = camera_box(c2w, max_depth)
    voxel = float(voxel_size)
    if not voxel > 0:
        raise ValueError("the voxel size must be positive")
    dims = tuple(max(1, int(math.ceil(float(s) / voxel - 1e-9))) for s in hi - lo)
    return tuple(float(v) for v in lo), dims


def write_ply(path, xyz, rgb):
    """A binary little-endian PLY of points: float x y z, uchar red green blue."""
    xyz = xyz.detach().cpu().numpy() if isinstance(xyz, torch.Tensor) else np.asarray(xyz)
    rgb = rgb.detach().cpu().numpy() if isinstance(rgb, torch.Tensor) else np.asarray(rgb)
    if xyz.ndim != 2 or xyz.shape[1] != 3 or rgb.shape != xyz.shape:
        raise ValueError(f"xyz and rgb must both be [N, 3], got {list(xyz.shape)} and {list(rgb.shape)}")
    rec = np.empty(len(xyz), dtype=[("xyz", "<f4", 3), ("rgb", "u1", 3)])
    rec["xyz"], rec["rgb"] = xyz, rgb
    header = ("ply\nformat binary_little_endian 1.0\nelement vertex {}\nproperty float x\nproperty float y\n"
              "property float z\nproperty uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n")
    with open(path, "wb") as f:
        f.write(header.format(len(xyz)).encode("ascii"))
        f.write(rec.tobytes())
