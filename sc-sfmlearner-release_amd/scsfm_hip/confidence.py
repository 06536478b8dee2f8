"""Depth consistency as a per-pixel confidence, and the fusion weighed by it, through libscsfm_conf.so
(include/scsfm_conf.h).  The training loss compares the depth a frame computes for a point with the depth its neighbour
predicts there, |D_computed - D_projected| / (D_computed + D_projected); one minus it is the self-discovered mask.  Here
the same quantity is taken at inference, between the fused frames, and every observation enters the volume with it as
its weight: what moved, was occluded or is simply wrong counts for less, or, below a floor, not at all.

    w = confidence.weights(disp, c2w, K, radius=1)                  # float32 [n, H, W], between 0 and 1
    vol.integrate(disp, images, c2w, K, weight=w)                   # or confidence.integrate(vol, ..., weight=w)

``disp`` is the disparity net's output [n, 1, H, W] (or [n, H, W]) of n frames in sequence order, ``c2w`` their poses,
float64 [n, 3, 4]; frame i is compared with the frames i - radius .. i + radius that exist.  Everything stays on the
device and nothing is copied to the host.  There is no torch fallback: without a HIP device or the library this raises,
and so do float64, CPU and non-contiguous tensors.
"""
from __future__ import annotations

import torch

from . import _lib
from .fusion import _check, _ptr, _stream, cameras

MAX_RADIUS = 4
REDUCE = {"mean": 0, "max": 1}


def _frames(name, t):
    d = _check(name, t, torch.float32)
    if d.dim() == 4 and d.shape[1] == 1:
        d = d[:, 0]
    if d.dim() != 3 or not d.numel():
        raise ValueError(f"{name} must be [n, 1, H, W] or [n, H, W], got {list(t.shape)}")
    return d


def _radius(radius):
    radius = int(radius)
    if not 1 <= radius <= MAX_RADIUS:
        raise ValueError(f"radius must be 1 .. {MAX_RADIUS}, got {radius}")
    return radius


def pair_cameras(c2w, K, radius):
    """c2w float64 [n, 3, 4] (or [n, 12]) and K float32 [3, 3] on the device -> the pair records float32
    [n, 2 radius, 16]: slot s of frame i holds the transform from its camera to the camera of frame i + o, o over
    -radius .. -1, 1 .. radius (rotation 9, translation 3), then fx, fy, cx, cy; sixteen zeros where there is no frame."""
    radius = _radius(radius)
    _check("c2w", c2w, torch.float64)
    if not c2w.numel() or c2w.numel() % 12 or c2w.shape[-1] not in (4, 12):
        raise ValueError(f"c2w must be [n, 3, 4] or [n, 12], got {list(c2w.shape)}")
    _check("K", K, torch.float32, (3, 3))
    if K.device != c2w.device:
        raise ValueError("the poses and the intrinsics must live on the same device")
    n = c2w.numel() // 12
    pair = torch.empty((n, 2 * radius, 16), dtype=torch.float32, device=c2w.device)
    _lib.get_conf().call("scsfm_conf_pairs", n, radius, _ptr(c2w), _ptr(K), _ptr(pair), _stream(c2w.device))
    return pair


def weights(disp_or_depth, c2w, K, radius=1, is_disp=True, max_depth=10.0, min_views=1, floor=0.0, reduce="mean"):
    """-> float32 [n, H, W]: the confidence of every pixel of n frames in sequence order, all in one launch.  A pixel
    whose own depth is not in (0, max_depth], or that fewer than ``min_views`` of its 2 ``radius`` neighbours can be
    compared with, gets 0; otherwise the mean (``reduce="mean"``, what the training loss averages) or the largest
    (``"max"``: one confirming neighbour is enough, which is kinder to occlusions) of 1 - |d - d'| / (d + d') over them,
    and 0 where that is below ``floor``."""
    d = _frames("disp_or_depth", disp_or_depth)
    n, H, W = d.shape
    if reduce not in REDUCE:
        raise ValueError(f"reduce must be one of {sorted(REDUCE)}, got {reduce!r}")
    pair = pair_cameras(c2w, K, radius)
    if pair.shape[0] != n:
        raise ValueError(f"{pair.shape[0]} poses for {n} frames")
    if pair.device != d.device:
        raise ValueError("the frames and the poses must live on the same device")
    out = torch.empty((n, H, W), dtype=torch.float32, device=d.device)
    _lib.get_conf().call("scsfm_conf_weights", n, pair.shape[1] // 2, H, W, _ptr(d), int(bool(is_disp)), _ptr(pair),
                         float(max_depth), int(min_views), float(floor), REDUCE[reduce], _ptr(out), _stream(d.device))
    return out


def integrate(volume, disp_or_depth, images, c2w, K, weight, is_disp=True, near=0.0, max_depth=10.0):
    """fusion.Volume.integrate with every observation weighed by ``weight`` float32 [F, H, W] (or [F, 1, H, W]): a pixel
    whose weight is not in (0, 1] is not fused, and a weight of all ones leaves the bits of the unweighted call.  In
    launches of ``volume.frames_per_launch``."""
    d = _frames("disp_or_depth", disp_or_depth)
    F, H, W = d.shape
    w = _frames("weight", weight)
    if tuple(w.shape) != (F, H, W):
        raise ValueError(f"weight must be {[F, H, W]}, got {list(weight.shape)}")
    if images is not None:
        _check("images", images, torch.float32, (F, 3, H, W))
    cam = cameras(c2w, K)
    if cam.shape[0] != F:
        raise ValueError(f"{cam.shape[0]} poses for {F} frames")
    if any(t.device != volume.planes.device for t in (d, w, cam) + (() if images is None else (images,))):
        raise ValueError("the frames, their weights and the poses must live on the volume's device")
    lib = _lib.get_conf()
    stream = _stream(volume.device)
    for f0 in range(0, F, volume.frames_per_launch):
        n = min(F, f0 + volume.frames_per_launch) - f0
        lib.call("scsfm_conf_integrate", *volume.dims, *volume.origin, volume.voxel, volume.trunc, float(near),
                 float(max_depth), volume.max_weight, n, H, W, _ptr(cam[f0:]), _ptr(d[f0:]), _ptr(w[f0:]),
                 int(bool(is_disp)), None if images is None else _ptr(images[f0:]), _ptr(volume.planes), stream)
