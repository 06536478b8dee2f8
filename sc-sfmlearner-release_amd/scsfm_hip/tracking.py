"""Frame-to-model tracking through libscsfm_track.so (include/scsfm_track.h): the poses of V frames are refined against the
fused volume by point-to-plane ICP, as KinectFusion aligns a frame before it fuses it.  The volume is cast from the guessed
poses (scsfm_hip.raycast), every pixel of a frame's depth is paired with the model pixel it projects to, 29 sums per frame
are reduced in a fixed order and a 6 x 6 system is solved and applied on the device: an iteration is two launches for all V
frames and nothing is copied to the host.

    vol = fusion.Volume(dims, origin, 0.05, device="cuda")
    vol.integrate(disp[:1], images[:1], c2w[:1], K)
    out = vol.track(disp[1:4], guess, K, is_disp=True, max_depth=10.0)        # or tracking.track(vol, ...)
    out.c2w            # float64 [V, 3, 4]: the refined poses, camera to world
    out.report         # float64 [V, iterations, 4]: pairs, sum of r^2, status, smallest pivot ratio -- before each update
    out.model_depth    # float32 [V, H, W], out.model_normal float32 [V, 3, H, W]: the cast the frames were aligned to
    out.state          # float64 [V, 7]: the unit quaternions (w, x, y, z) and centres behind c2w

A status of 1 (fewer than ``min_pairs`` pairs) or 2 (a rank-deficient system) leaves the pose as it was; ``kept_guess``
tells the frames that never moved.  ``align`` is the same on maps cast before.  There is no torch fallback: without a HIP
device or the library this raises, and so do float64 depths, CPU and non-contiguous tensors.
"""
from __future__ import annotations

from typing import NamedTuple

import torch

from . import _lib, raycast
from .raycast import _check, _ptr, _stream

MAX_ITERATIONS = 64


class Track(NamedTuple):
    c2w: torch.Tensor
    report: torch.Tensor
    model_depth: torch.Tensor
    model_normal: torch.Tensor
    state: torch.Tensor


def kept_guess(report):
    """report [V, iterations, 4] -> bool [V]: the frames whose every iteration reported a non-zero status"""
    return (report[:, :, 2] != 0).all(dim=1)


def _frames(depth_or_disp):
    d = _check("depth_or_disp", depth_or_disp, torch.float32)
    if d.dim() == 4 and d.shape[1] == 1:
        d = d[:, 0]
    if d.dim() != 3 or not d.numel():
        raise ValueError(f"depth_or_disp must be [V, 1, H, W] or [V, H, W], got {list(depth_or_disp.shape)}")
    return d


def _posed_frames(depth_or_disp, guess):
    """The frames of ``align``, here and in scsfm_hip.similarity, as [V, H, W], with their poses checked."""
    d = _frames(depth_or_disp)
    _check("guess", guess, torch.float64)
    if guess.numel() != 12 * len(d) or guess.shape[-1] not in (4, 12):
        raise ValueError(f"guess must be [{len(d)}, 3, 4], got {list(guess.shape)}")
    return d


def _check_maps(d, guess, K, ref_view, model_depth, model_normal):
    """What ``align`` asks of the intrinsics and the model maps of the frames ``d``, and that all share a device."""
    V, H, W = d.shape
    _check("K", K, torch.float32, (3, 3))
    _check("ref_view", ref_view, torch.float32, (V, 16))
    _check("model_depth", model_depth, torch.float32, (V, H, W))
    _check("model_normal", model_normal, torch.float32, (V, 3, H, W))
    if any(t.device != d.device for t in (guess, K, ref_view, model_depth, model_normal)):
        raise ValueError("the frames, the poses and the model maps must live on the same device")


def align(depth_or_disp, guess, K, ref_view, model_depth, model_normal, *, is_disp=True, near=0.0, max_depth=10.0,
          iterations=10, max_dist, min_pairs=64):
    """Aligns V frames -- the nets' disparity (``is_disp``) or a depth, float32 [V, 1, H, W] or [V, H, W] -- from the
    poses ``guess`` (float64 [V, 3, 4], camera to world) to the model maps ``model_depth`` [V, H, W] and ``model_normal``
    [V, 3, H, W] that raycast.cast wrote for the view records ``ref_view`` (float32 [V, 16], raycast.views) -> Track.
    A pair is dropped when frame and model point are further apart than ``max_dist``."""
    d = _posed_frames(depth_or_disp, guess)
    _check_maps(d, guess, K, ref_view, model_depth, model_normal)
    (V, H, W), dev = d.shape, d.device
    iterations, min_pairs = int(iterations), int(min_pairs)
    if not 1 <= iterations <= MAX_ITERATIONS:
        raise ValueError(f"iterations must be 1 .. {MAX_ITERATIONS}, got {iterations}")
    if min_pairs < 6:
        raise ValueError("min_pairs must be at least 6: a pose has six degrees of freedom")
    lib = _lib.get_track()
    n = lib.size("scsfm_track_ws_bytes", V, H, W)
    if not n:
        raise ValueError(f"{V} frames of {H} x {W} are refused: their sizes' products must stay below 2^31")
    stream = _stream(dev)
    state = torch.empty((V, 7), dtype=torch.float64, device=dev)
    est = torch.empty((V, 16), dtype=torch.float32, device=dev)
    ws = torch.empty(n // 8, dtype=torch.float64, device=dev)
    report = torch.empty((V, iterations, 4), dtype=torch.float64, device=dev)
    c2w = torch.empty((V, 3, 4), dtype=torch.float64, device=dev)
    lib.call("scsfm_track_init", V, _ptr(guess), _ptr(K), _ptr(state), _ptr(est), stream)
    lib.call("scsfm_track_iterate", V, H, W, _ptr(d), int(bool(is_disp)), float(near), float(max_depth), _ptr(ref_view),
             _ptr(model_depth), _ptr(model_normal), float(max_dist), min_pairs, iterations, _ptr(state), _ptr(est),
             _ptr(ws), _ptr(report), stream)
    lib.call("scsfm_track_poses", V, _ptr(state), _ptr(c2w), stream)
    return Track(c2w, report, model_depth, model_normal, state)


def track(volume, depth_or_disp, guess, K, *, is_disp=True, near=0.0, max_depth=10.0, iterations=10, max_dist=None,
          min_pairs=64, step=None, mask=None):
    """Casts ``volume`` (a fusion.Volume) from the V poses ``guess`` -- min_weight 1, since a model of one frame must
    already be trackable; normals on, colour and shade off; to a depth of max_depth + volume.trunc; ``step`` and ``mask``
    as raycast.cast takes them -- and aligns the frames to that cast (see ``align``) -> Track.  ``max_dist`` defaults to
    the volume's truncation distance."""
    d = _frames(depth_or_disp)
    _check("guess", guess, torch.float64)
    cast = raycast.cast(volume, guess, K, d.shape[1:], near, max_depth + volume.trunc, step=step, min_weight=1.0,
                        cull=True, normals=True, colour=False, shade=False, mask=mask)
    return align(d, guess, K, raycast.views(guess, K), cast.depth, cast.normal, is_disp=is_disp, near=near,
                 max_depth=max_depth, iterations=iterations, max_dist=volume.trunc if max_dist is None else max_dist,
                 min_pairs=min_pairs)
