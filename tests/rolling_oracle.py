"""include/scsfm_roll.h restated in numpy, on top of tests/fusion_oracle.py: the shift of the five planes, the extraction
of the crossings that leave with it, the lattice's origin and the policy that places the window.  The yardstick of
tests/test_rolling_hostsim.py and tests/test_gpu_rolling.py, which compare the kernels with it bit for bit.  Test
infrastructure only."""
from __future__ import annotations

import math

import numpy as np

import fusion_oracle as O

f32 = np.float32


def shift_planes(planes, s):
    """planes [5, nz, ny, nx] -> the same shape: voxel (x, y, z) takes the bits of voxel (x + sx, y + sy, z + sz) where that
    lies inside the volume and 0.0f elsewhere (moved as uint32: NaN payloads and denormals pass unchanged)"""
    src = np.ascontiguousarray(planes, np.float32).view(np.uint32)
    dst = np.zeros_like(src)
    _, nz, ny, nx = src.shape
    sel_d, sel_s = [slice(None)], [slice(None)]
    for n, k in ((nz, s[2]), (ny, s[1]), (nx, s[0])):
        lo, hi = max(0, -k), min(n, n - k)      # the dst indices whose source i + k lies in [0, n)
        if lo >= hi:
            return dst.view(np.float32)
        sel_d.append(slice(lo, hi))
        sel_s.append(slice(lo + k, hi + k))
    dst[tuple(sel_d)] = src[tuple(sel_s)]
    return dst.view(np.float32)


def keep_box(dims, s):
    """the old voxels that survive a move by s: per axis [max(0, s), min(n, n + s)) -> (x0, x1, y0, y1, z0, z1)"""
    out = []
    for n, k in zip(dims, s):
        out += [max(0, k), min(n, n + k)]
    return tuple(out)


def origin_at(origin0, offset, voxel):
    """per axis fl(origin0 + fl(float(k) s)), fp32"""
    return tuple(f32(o) + f32(k) * f32(voxel) for o, k in zip(origin0, offset))


def leaves(vol, box, min_weight=1.0):
    """-> bool [N] over vol.crossings(min_weight): voxel a or voxel b of the crossing's edge lies outside the keep box"""
    nx, ny, nz = vol.dims
    a, axis = vol.crossings(min_weight)
    ia = np.stack([a % nx, (a // nx) % ny, a // (nx * ny)], axis=1)
    ib = ia.copy()
    ib[np.arange(len(a)), axis] += 1
    lo, hi = np.array(box[0::2]), np.array(box[1::2])
    in_a = ((ia >= lo) & (ia < hi)).all(axis=1)
    in_b = ((ib >= lo) & (ib < hi)).all(axis=1)
    return ~(in_a & in_b)


def leaving(vol, box, min_weight=1.0):
    """the oracle's filter of fusion_oracle.Volume.extract -> (xyz, rgb, the chunks' counts int32)"""
    xyz, rgb, _ = vol.extract(min_weight)
    out = leaves(vol, box, min_weight)
    a, _ = vol.crossings(min_weight)
    nvox = int(np.prod(vol.dims))
    counts = np.bincount(a[out] // O.CHUNK, minlength=(nvox + O.CHUNK - 1) // O.CHUNK).astype(np.int32)
    return xyz[out], rgb[out], counts


def shift_for(centre, origin0, offset, dims, voxel, step):
    """the policy, float64, per axis: cell = floor((centre - origin0) / voxel) - offset, off = cell - dims // 2,
    shift = trunc(off / step) * step"""
    out = []
    for c, o, k, n in zip(centre, origin0, offset, dims):
        cell = math.floor((float(c) - float(o)) / float(voxel)) - k
        off = cell - n // 2
        out.append(int(off / step) * step)
    return tuple(out)


def initial_origin(centre, dims, voxel):
    return tuple(float(c) - (n // 2 + 0.5) * float(voxel) for c, n in zip(centre, dims))


class RollingVolume(O.Volume):
    """fusion_oracle.Volume whose origin is origin_at(origin0, offset, voxel)"""

    def __init__(self, dims, origin0, voxel_size, trunc=None, max_weight=64.0):
        super().__init__(dims, origin0, voxel_size, trunc, max_weight)
        self.origin0 = self.origin
        self.offset = (0, 0, 0)

    def shift(self, s, min_weight=1.0):
        s = tuple(int(k) for k in s)
        xyz, rgb, _ = leaving(self, keep_box(self.dims, s), min_weight)
        self.planes = shift_planes(self.planes, s)
        self.offset = tuple(k + d for k, d in zip(self.offset, s))
        self.origin = origin_at(self.origin0, self.offset, self.voxel)
        return xyz, rgb
