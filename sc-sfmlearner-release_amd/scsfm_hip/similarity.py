"""Frame-to-model tracking with a scale through libscsfm_sim3.so (include/scsfm_sim3.h): scsfm_hip.tracking's alignment with
a seventh degree of freedom, the scale of the frame's own depth.  The nets' depth is only softly scale-consistent along a
sequence, and a rigid tracker trades a frame's scale error for a wrong pose; here every frame carries a scale sigma, its
depth enters as sigma times the prediction, and the 7 x 7 system of an iteration is solved with the scale last, so that its
pivot alone decides whether the scale is solved or held at its value -- a frame that sees nothing but planes takes the
rigid step, bit for bit (the two libraries compile one core, csrc_icp/scsfm_icp.h).  37 sums per frame are reduced in a
fixed order; an iteration is two launches for all V frames and nothing is copied to the host.

    vol = fusion.Volume(dims, origin, 0.05, device="cuda")
    vol.integrate(disp[:1], images[:1], c2w[:1], K)
    out = vol.track_scaled(disp[1:4], guess, scale0, K, is_disp=True, max_depth=10.0)   # or similarity.track(vol, ...)
    out.c2w            # float64 [V, 3, 4]: the refined poses, camera to world
    out.scale          # float64 [V]: the refined scales
    out.report         # float64 [V, iterations, 6]: pairs, sum of r^2, status, smallest pose pivot ratio, scale pivot
                       # ratio, scale -- before each update
    out.model_depth    # float32 [V, H, W], out.model_normal float32 [V, 3, H, W]: the cast the frames were aligned to
    out.state          # float64 [V, 8]: the unit quaternions (w, x, y, z), centres and scales behind c2w and scale
    depth = similarity.scaled_depth(disp[1:4], out.scale, is_disp=True)   # what the tracker saw: integrate it as a depth

A status of 1 (fewer than ``min_pairs`` pairs) or 2 (a rank-deficient system, or a scale that is not positive and finite)
leaves pose and scale as they were; ``kept_guess`` tells the frames that never moved.  A status of 3 moved the pose and
held the scale; ``held_scale`` tells the frames whose scale was never solved.  ``align`` is the same on maps cast before.
There is no torch fallback: without a HIP device or the library this raises, and so do float64 depths, CPU and
non-contiguous tensors.
"""
from __future__ import annotations

from typing import NamedTuple

import torch

from . import _lib, raycast
from .raycast import _check, _ptr, _stream
from .tracking import _check_maps, _frames, _posed_frames

MAX_ITERATIONS = 64
# The smallest ratio of the scale's LDL^T pivot to the largest diagonal entry of the 7 x 7 matrix at which the scale is
# solved.  It comes from a measurement with a float64 prototype of the design on tests/_track_cases.py's room, three frames
# each at 12 x 20 and 37 x 61, ten iterations, guesses off by a voxel and a degree: with the sphere in the room's corner,
# where the scale is observable, the ratio was 3.1e-2 .. 4.1e-2 at its smallest; in the room of the three planes alone,
# where n . u and n . t are both constant on each plane and a scale solved anyway runs away (one frame to 0.05 in four
# iterations), it was 7e-5 .. 4.1e-4.  2e-3 is 15 times below the smallest ratio of the observable room and 5 times above
# the largest of the planes-only room.  The restatement of the finished header (tests/sim3_oracle.py, on
# tests/_sim3_cases.py) leaves no less room on either side: 8.2e-2 at the smallest with the sphere (6.7e-2 with holes cut
# into the model maps), 4.6e-5 .. 1.3e-4 with the planes alone, whether the scale is held there or solved all the same
# (three frames then end at 0.76 .. 0.82 after four iterations).
MIN_SCALE_PIVOT = 2e-3


class Track(NamedTuple):
    c2w: torch.Tensor
    scale: torch.Tensor
    report: torch.Tensor
    model_depth: torch.Tensor
    model_normal: torch.Tensor
    state: torch.Tensor


def kept_guess(report):
    """report [V, iterations, 6] -> bool [V]: the frames whose every iteration reported status 1 or 2 (pose and scale are
    the guess's)"""
    status = report[:, :, 2]
    return ((status == 1) | (status == 2)).all(dim=1)


def held_scale(report):
    """report [V, iterations, 6] -> bool [V]: the frames with no iteration of status 0 (the scale is the one they came
    with)"""
    return (report[:, :, 2] != 0).all(dim=1)


def _scales(name, scale, V, dev):
    _check(name, scale, torch.float64, (V,))
    if scale.device != dev:
        raise ValueError("the frames and the scales must live on the same device")
    return scale


def scaled_depth(depth_or_disp, scale, is_disp=True):
    """The depth the tracker saw of V frames (float32 [V, 1, H, W] or [V, H, W], the nets' disparity with ``is_disp``) at
    the scales ``scale`` (float64 [V]): float32(scale) times the depth, bit for bit step 1 of include/scsfm_sim3.h ->
    float32 of the input's shape.  It is a depth: integrate it with is_disp=False."""
    d = _frames(depth_or_disp)
    V, H, W = d.shape
    _scales("scale", scale, V, d.device)
    out = torch.empty_like(d)
    sigma_f = scale.float()      # (one rounding, as the state's sigma_f)
    _lib.get_sim3().call("scsfm_sim3_scale", V, H, W, _ptr(d), int(bool(is_disp)), _ptr(sigma_f), _ptr(out),
                         _stream(d.device))
    return out.reshape(depth_or_disp.shape)


def align(depth_or_disp, guess, scale0, K, ref_view, model_depth, model_normal, *, is_disp=True, near=0.0, max_depth=10.0,
          iterations=10, max_dist, min_pairs=64, min_scale_pivot=MIN_SCALE_PIVOT):
    """Aligns V frames -- the nets' disparity (``is_disp``) or a depth, float32 [V, 1, H, W] or [V, H, W] -- from the
    poses ``guess`` (float64 [V, 3, 4], camera to world) and the scales ``scale0`` (float64 [V]) to the model maps
    ``model_depth`` [V, H, W] and ``model_normal`` [V, 3, H, W] that raycast.cast wrote for the view records ``ref_view``
    (float32 [V, 16], raycast.views) -> Track.  A pair is dropped when frame and model point are further apart than
    ``max_dist``.  The scale of a frame is solved in an iteration whose scale pivot ratio is above ``min_scale_pivot``
    (``math.inf``: never) and held otherwise."""
    d = _posed_frames(depth_or_disp, guess)
    (V, H, W), dev = d.shape, d.device
    _scales("scale0", scale0, V, dev)
    _check_maps(d, guess, K, ref_view, model_depth, model_normal)
    iterations, min_pairs, min_scale_pivot = int(iterations), int(min_pairs), float(min_scale_pivot)
    if not 1 <= iterations <= MAX_ITERATIONS:
        raise ValueError(f"iterations must be 1 .. {MAX_ITERATIONS}, got {iterations}")
    if min_pairs < 7:
        raise ValueError("min_pairs must be at least 7: a pose and a scale have seven degrees of freedom")
    if not min_scale_pivot > 0:
        raise ValueError(f"min_scale_pivot must be positive (math.inf: the scale is never solved), got {min_scale_pivot}")
    lib = _lib.get_sim3()
    n = lib.size("scsfm_sim3_ws_bytes", V, H, W)
    if not n:
        raise ValueError(f"{V} frames of {H} x {W} are refused: their sizes' products must stay below 2^31")
    stream = _stream(dev)
    state = torch.empty((V, 8), dtype=torch.float64, device=dev)
    est = torch.empty((V, 16), dtype=torch.float32, device=dev)
    sigma_f = torch.empty((V,), dtype=torch.float32, device=dev)
    ws = torch.empty(n // 8, dtype=torch.float64, device=dev)
    report = torch.empty((V, iterations, 6), dtype=torch.float64, device=dev)
    c2w = torch.empty((V, 3, 4), dtype=torch.float64, device=dev)
    scale = torch.empty((V,), dtype=torch.float64, device=dev)
    lib.call("scsfm_sim3_init", V, _ptr(guess), _ptr(scale0), _ptr(K), _ptr(state), _ptr(est), _ptr(sigma_f), stream)
    lib.call("scsfm_sim3_iterate", V, H, W, _ptr(d), int(bool(is_disp)), float(near), float(max_depth), _ptr(ref_view),
             _ptr(model_depth), _ptr(model_normal), float(max_dist), min_pairs, min_scale_pivot, iterations, _ptr(state),
             _ptr(est), _ptr(sigma_f), _ptr(ws), _ptr(report), stream)
    lib.call("scsfm_sim3_poses", V, _ptr(state), _ptr(c2w), _ptr(scale), stream)
    return Track(c2w, scale, report, model_depth, model_normal, state)


def track(volume, depth_or_disp, guess, scale0, K, *, is_disp=True, near=0.0, max_depth=10.0, iterations=10,
          max_dist=None, min_pairs=64, min_scale_pivot=MIN_SCALE_PIVOT, step=None, mask=None):
    """Casts ``volume`` (a fusion.Volume) from the V poses ``guess`` exactly as tracking.track does -- min_weight 1,
    normals on, colour and shade off, to a depth of max_depth + volume.trunc; ``step`` and ``mask`` as raycast.cast takes
    them -- and aligns the frames to that cast (see ``align``) -> Track.  ``max_dist`` defaults to the volume's truncation
    distance."""
    d = _frames(depth_or_disp)
    _check("guess", guess, torch.float64)
    cast = raycast.cast(volume, guess, K, d.shape[1:], near, max_depth + volume.trunc, step=step, min_weight=1.0,
                        cull=True, normals=True, colour=False, shade=False, mask=mask)
    return align(d, guess, scale0, K, raycast.views(guess, K), cast.depth, cast.normal, is_disp=is_disp, near=near,
                 max_depth=max_depth, iterations=iterations, max_dist=volume.trunc if max_dist is None else max_dist,
                 min_pairs=min_pairs, min_scale_pivot=min_scale_pivot)
