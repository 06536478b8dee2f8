"""Ray casting of a fused volume through libscsfm_cast.so (include/scsfm_cast.h): the depth the model has from a camera
pose, its world normals, a colour picture and a headlight-shaded picture, one thread per pixel marching the TSDF.

    vol = fusion.Volume(dims, origin, 0.05, device="cuda")
    vol.integrate(disp, images, c2w, K, is_disp=True, max_depth=10.0)
    out = vol.raycast(c2w, K, (H, W), near=0.0, far=10.0 + vol.trunc, min_weight=2)   # or raycast.cast(vol, ...)
    out.depth      # float32 [V, H, W]: the units and layout of 1 / disp, 0 where no surface is seen
    out.normal     # float32 [V, 3, H, W], world axes, towards free space      (None with normals=False)
    out.rgb        # uint8 [V, H, W, 3], ready for a PNG                        (None with colour=False)
    out.shade      # uint8 [V, H, W]: 255 cos of the angle between ray and normal  (None with shade=False)

Everything stays on the device and nothing is copied to the host.  The brick mask (one byte per 8 x 8 x 8 voxels) lets the
march skip the samples that cannot be inside the surface; it changes no bit of the result (``cull=False`` evaluates every
sample).  There is no torch fallback: without a HIP device or the library this raises, and so do float64, CPU and
non-contiguous tensors.
"""
from __future__ import annotations

import ctypes
import math
from typing import NamedTuple, Optional

import torch

from . import _lib

MAX_STEPS = 1 << 20


class Cast(NamedTuple):
    depth: torch.Tensor
    normal: Optional[torch.Tensor]
    rgb: Optional[torch.Tensor]
    shade: Optional[torch.Tensor]


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream(device):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _check(name, t, dtype, shape=None):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch tensor, got {type(t).__name__}")
    if not t.is_cuda:
        raise TypeError(f"{name} must live on the HIP device (the ray-cast kernels have no CPU fallback)")
    if t.dtype != dtype:
        raise TypeError(f"{name} must be {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name} must be {list(shape)}, got {list(t.shape)}")
    return t


def _planes(volume):
    """the five planes [5, nz, ny, nx] of a fusion.Volume (or the tensor itself), checked"""
    planes = _check("the volume's planes", getattr(volume, "planes", volume), torch.float32)
    if planes.dim() != 4 or planes.shape[0] != 5:
        raise ValueError(f"the volume's planes must be [5, nz, ny, nx], got {list(planes.shape)}")
    return planes


def views(c2w, K):
    """c2w float64 [V, 3, 4] (or [V, 12]) and K float32 [3, 3] on the device -> the kernels' view records, float32
    [V, 16]: the camera-to-world matrix (9), the centre (3), fx, fy, cx, cy."""
    _check("c2w", c2w, torch.float64)
    if c2w.numel() % 12 or c2w.shape[-1] not in (4, 12):
        raise ValueError(f"c2w must be [V, 3, 4] or [V, 12], got {list(c2w.shape)}")
    _check("K", K, torch.float32, (3, 3))
    n = c2w.numel() // 12
    view = torch.empty((n, 16), dtype=torch.float32, device=c2w.device)
    if n:
        _lib.get_cast().call("scsfm_cast_views", n, _ptr(c2w), _ptr(K), _ptr(view), _stream(c2w.device))
    return view


def brick_mask(volume, min_weight=1.0):
    """-> uint8 [ceil(nz / 8), ceil(ny / 8), ceil(nx / 8)] on the device: 1 where some voxel of the brick's nine-wide range
    has weight >= min_weight and tsdf < 0"""
    planes = _planes(volume)
    _, nz, ny, nx = planes.shape
    lib = _lib.get_cast()
    n = lib.size("scsfm_cast_mask_bytes", nx, ny, nz)
    if not n:
        raise ValueError(f"a volume of {(nx, ny, nz)} voxels is refused: every size must be positive and their product "
                         f"at most 2^29")
    mask = torch.empty((-(-nz // 8), -(-ny // 8), -(-nx // 8)), dtype=torch.uint8, device=planes.device)
    assert mask.numel() == n
    lib.call("scsfm_cast_mask", nx, ny, nz, _ptr(planes), float(min_weight), _ptr(mask), _stream(planes.device))
    return mask


def cast(volume, c2w, K, hw, near, far, step=None, min_weight=1.0, cull=True, normals=True, colour=True, shade=True,
         mask=None):
    """Casts the V poses ``c2w`` (float64 [V, 3, 4], camera to world) with the intrinsics ``K`` (float32 [3, 3]) of
    ``hw`` = (H, W) pixels through ``volume`` (a fusion.Volume) -> Cast(depth, normal, rgb, shade), device tensors; an
    output that is switched off is None and is not computed.

    The march samples the depths near, near + step, ... below ``far``: ``step`` defaults to the voxel size and
    n_steps = ceil((far - near) / step).  A surface is found between two consecutive samples on either side of it, so
    the world length of a step, step |w| with w the ray's direction at camera depth 1 (|w| = sqrt(1 + dx^2 + dy^2) for a
    rotation: 1 on the axis, larger towards the picture's corners), must stay below the volume's truncation distance, or
    a thin band can be stepped over; the default step with the default truncation of three voxels allows |w| < 3.
    ``cull`` builds the brick mask first (``mask``: one built before by brick_mask for this volume and min_weight) and
    changes no bit of the result."""
    planes = _planes(volume)
    origin, voxel = volume.origin, volume.voxel
    _, nz, ny, nx = planes.shape
    H, W = (int(v) for v in hw)
    view = views(c2w, K)
    V = view.shape[0]
    if view.device != planes.device:
        raise ValueError("the poses and the volume must live on the same device")
    step = float(voxel if step is None else step)
    near, far = float(near), float(far)
    if not (step > 0 and math.isfinite(step) and near >= 0 and math.isfinite(far) and far > near):
        raise ValueError("the march needs 0 <= near < far and step > 0, all finite")
    n_steps = int(math.ceil((far - near) / step))
    if not 1 <= n_steps <= MAX_STEPS:
        raise ValueError(f"{n_steps} steps between near and far: at most 2^20 are allowed (choose a larger step)")
    if H <= 0 or W <= 0 or V <= 0:
        raise ValueError("a cast needs at least one view and a picture of at least one pixel")
    if mask is None and cull:
        mask = brick_mask(volume, min_weight)
    elif mask is not None:
        _check("mask", mask, torch.uint8)
        if mask.numel() != -(-nz // 8) * -(-ny // 8) * -(-nx // 8):
            raise ValueError("mask is not the brick mask of this volume")
    dev = planes.device
    depth = torch.empty((V, H, W), dtype=torch.float32, device=dev)
    normal = torch.empty((V, 3, H, W), dtype=torch.float32, device=dev) if normals else None
    rgb = torch.empty((V, H, W, 3), dtype=torch.uint8, device=dev) if colour else None
    sh = torch.empty((V, H, W), dtype=torch.uint8, device=dev) if shade else None
    _lib.get_cast().call("scsfm_cast_cast", nx, ny, nz, *origin, voxel, _ptr(planes), float(min_weight), near, step,
                         n_steps, V, H, W, _ptr(view), _ptr(mask), _ptr(depth), _ptr(normal), _ptr(rgb), _ptr(sh),
                         _stream(dev))
    return Cast(depth, normal, rgb, sh)
