"""A truncated signed distance volume of fixed size that follows the camera, through libscsfm_roll.so
(include/scsfm_roll.h): KinectFusion's moving volume.  What falls out behind is turned into surface points and forgotten,
so memory is fixed by what a frame can see, not by the length of the path.

    origin0 = initial_origin(centre, dims, 0.05)
    vol = RollingVolume(dims, origin0, 0.05, device="cuda")
    for each batch:
        s = shift_for(centre, vol.origin0, vol.offset, vol.dims, vol.voxel, step=8)
        if any(s):
            xyz, rgb = vol.shift(s, min_weight=2)        # the points that leave, on the device
        vol.integrate(disp, images, c2w, K, is_disp=True, max_depth=10.0)
    xyz, rgb = vol.extract(min_weight=2)                 # what is still inside

The lattice is fixed: the window's corner is always ``origin0 + offset * voxel`` with an integer ``offset``, computed in
fp32 from the offset every time (``origin_at``) and never accumulated, so a voxel of the world has the same centre in every
window that holds it, and the streamed points with the final extraction are the points of one big volume on that lattice.
There is no torch fallback: without a HIP device or the library this raises, and so do float64, CPU and non-contiguous
tensors.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import _lib
from . import fusion
from .fusion import _ptr, _stream


def origin_at(origin0, offset, voxel_size):
    """The corner of the window at ``offset``: per axis fl(origin0 + fl(float(k) s)) in fp32 -> three floats."""
    s = np.float32(voxel_size)
    return tuple(float(np.float32(o) + np.float32(k) * s) for o, k in zip(origin0, offset))


def keep_box(dims, shift):
    """The old voxels that survive a move by ``shift``: per axis [max(0, s), min(n, n + s)) -> (x0, x1, y0, y1, z0, z1)."""
    box = []
    for n, s in zip(dims, shift):
        box += [max(0, int(s)), min(int(n), int(n) + int(s))]
    return tuple(box)


def shift_for(centre, origin0, offset, dims, voxel, step):
    """The policy: how far the window of ``dims`` voxels at ``offset`` moves for a camera at ``centre`` -> three ints.
    Pure Python, float64, per axis: cell = floor((centre - origin0) / voxel) - offset is the camera's cell in the window,
    off = cell - dims // 2 its distance from the central cell, and the move is trunc(off / step) * step: whole multiples of
    ``step``, once the camera's cell is ``step`` or more voxels from the central one."""
    step = int(step)
    if step < 1:
        raise ValueError("step must be at least 1")
    out = []
    for c, o, k, n in zip(centre, origin0, offset, dims):
        cell = math.floor((float(c) - float(o)) / float(voxel)) - int(k)
        off = cell - int(n) // 2
        out.append(math.trunc(off / step) * step)
    return tuple(out)


def initial_origin(centre, dims, voxel):
    """origin0 that puts ``centre`` in the middle of the central cell: centre - (dims // 2 + 0.5) * voxel -> three floats"""
    return tuple(float(c) - (int(n) // 2 + 0.5) * float(voxel) for c, n in zip(centre, dims))


class RollingVolume(fusion.Volume):
    """fusion.Volume whose corner moves: ``origin0`` is fixed, ``offset`` (three ints, in voxels) is cumulative, and
    ``origin`` is origin_at(origin0, offset, voxel).  It holds two plane buffers, ping-pong (``nbytes``: 40 bytes a voxel);
    ``planes`` is the current one.  ``planes`` and ``origin`` are what every other wrapper reads, so integrate (plain and
    ``weight=``), extract, track, raycast and raycast.brick_mask work on it unchanged -- but whatever was derived from the
    planes before a shift is stale after it: a brick mask has to be built again."""

    def __init__(self, dims, origin0, voxel_size, trunc=None, max_weight=64.0, device="cuda",
                 frames_per_launch=fusion.FRAMES_PER_LAUNCH):
        if torch.device(device).type != "cuda":
            raise TypeError("a rolling volume must live on the HIP device (the kernels have no CPU fallback)")
        super().__init__(dims, origin0, voxel_size, trunc, max_weight, device, frames_per_launch)
        self.origin0 = self.origin
        self.offset = (0, 0, 0)
        self._roll = _lib.get_roll()
        self._spare = torch.zeros_like(self.planes)

    @property
    def nbytes(self):
        return 2 * self.planes.numel() * 4

    def leaving(self, shift, min_weight=1.0, capacity=None):
        """-> (xyz float32 [N, 3], rgb uint8 [N, 3]) on the device: the crossings, in extract()'s order, of the edges with
        an end outside keep_box(dims, shift), at the current origin.  One int crosses to the host."""
        box = keep_box(self.dims, shift)
        n = self._roll.size("scsfm_roll_ws_bytes", *self.dims)
        ws = torch.empty(n // 4, dtype=torch.int32, device=self.device)
        stream = _stream(self.device)
        self._roll.call("scsfm_roll_count", *self.dims, *box, _ptr(self.planes), float(min_weight), _ptr(ws), n, stream)
        total = int(ws[0].item())
        cap = total if capacity is None else int(capacity)
        xyz = torch.empty((cap, 3), dtype=torch.float32, device=self.device)
        rgb = torch.empty((cap, 3), dtype=torch.uint8, device=self.device)
        self._roll.call("scsfm_roll_extract", *self.dims, *self.origin, self.voxel, *box, _ptr(self.planes),
                        float(min_weight), _ptr(ws), n, cap, _ptr(xyz) if cap else None, _ptr(rgb) if cap else None, stream)
        return xyz, rgb

    def move(self, shift):
        """The planes moved by ``shift`` voxels into the other buffer, which becomes ``planes``; what enters is empty."""
        shift = tuple(int(s) for s in shift)
        self._roll.call("scsfm_roll_shift", *self.dims, *shift, _ptr(self.planes), _ptr(self._spare), _stream(self.device))
        self.planes, self._spare = self._spare, self.planes
        self.offset = tuple(k + s for k, s in zip(self.offset, shift))
        self.origin = origin_at(self.origin0, self.offset, self.voxel)

    def shift(self, shift, min_weight=1.0):
        """Moves the window by ``shift`` = (sx, sy, sz) voxels -> the surface points that leave (leaving()): counts and
        extracts them at the current origin, shifts into the other buffer and swaps, then updates ``offset`` and
        ``origin``."""
        shift = tuple(int(s) for s in shift)
        if len(shift) != 3:
            raise ValueError("a shift has three entries")
        out = self.leaving(shift, min_weight)
        self.move(shift)
        return out
