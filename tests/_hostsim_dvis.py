"""Compiles the depth-visualisation kernels (sc-sfmlearner-release_amd/csrc_dvis/*.hip), unchanged, against the host
simulator (tests/hostsim/hip/hip_runtime.h) with g++ into tests/hostsim/_build_dvis/, and runs the C ABI of
include/scsfm_dvis.h on HOST pointers.  Test infrastructure only; never loaded by the product."""
from __future__ import annotations

import ctypes
import functools
import os

import numpy as np

from hostsim import library
from scsfm_hip import depth_vis
from scsfm_hip._lib import DVIS_ABI_VERSION, DVIS_HEADER, CLib

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(ROOT, "sc-sfmlearner-release_amd", "csrc_dvis")
HOSTSIM = os.path.join(HERE, "hostsim")
OUT = os.path.join(HOSTSIM, "_build_dvis")
LIB = os.path.join(OUT, "libscsfm_dvis_hostsim.so")


def build(force=False):
    return library.build("dvis", force, dep=os.path.abspath(__file__))


@functools.lru_cache(maxsize=1)
def lib():
    return CLib(build(), DVIS_HEADER, DVIS_ABI_VERSION, "scsfm_dvis_")


def _ptr(a):
    return ctypes.c_void_p(a.ctypes.data)


class Ragged:
    """numpy twin of scsfm_hip.depth_vis.Ragged.  ``shift`` moves every offset by that many elements, off the
    multiples of 4.  The buffer starts as NaN with a guard band after the last map."""

    def __init__(self, sizes, dtype, shift=0):
        self.sizes = np.asarray(sizes, np.int64).reshape(-1, 2)
        self.hw = self.sizes[:, 0] * self.sizes[:, 1]
        slot = (self.hw + 3) // 4 * 4
        self.off = (np.concatenate([[0], np.cumsum(slot)[:-1]]) + shift).astype(np.int64)
        self.total = int(self.off[-1] + self.hw[-1])
        self.max_hw = int(self.hw.max())
        self.buf = np.full(self.total + 16, np.nan, dtype)
        self.h = self.sizes[:, 0].astype(np.int32)
        self.w = self.sizes[:, 1].astype(np.int32)

    def __len__(self):
        return len(self.sizes)

    def map(self, i):
        return self.buf[self.off[i]:self.off[i] + self.hw[i]].reshape(self.sizes[i])

    @classmethod
    def pack(cls, maps, shift=0):
        r = cls([m.shape for m in maps], maps[0].dtype, shift)
        for i, m in enumerate(maps):
            r.map(i)[...] = m
        return r

    def untouched(self):
        """True when every element outside the maps still holds its NaN."""
        keep = np.ones(len(self.buf), bool)
        for o, n in zip(self.off, self.hw):
            keep[o:o + n] = False
        return bool(np.isnan(self.buf[keep]).all())


def scaled_depths(pred, ratios, sizes, rdt, shift=0):
    pred = np.ascontiguousarray(pred)
    N, h, w = pred.shape
    out = Ragged(sizes, rdt, shift)
    ratio = np.asarray(ratios, np.float64).astype(rdt)
    lib().call("scsfm_dvis_scaled_depth", N, h, w, int(pred.dtype == np.float64), _ptr(pred),
               int(np.dtype(rdt) == np.float64), _ptr(ratio), _ptr(out.off), _ptr(out.h), _ptr(out.w), out.max_hw,
               _ptr(out.buf), None)
    assert out.untouched()
    return out


def depth_range(maps, shift=0):
    r = maps if isinstance(maps, Ragged) else Ragged.pack(maps, shift)
    T = r.buf.dtype.type
    f64 = int(r.buf.dtype == np.float64)
    idx = [depth_vis.percentile_index(int(n), T) for n in r.hw]
    lo, hi = np.array([i[0] for i in idx], np.int32), np.array([i[1] for i in idx], np.int32)
    t = np.array([i[2] for i in idx], T)
    nbytes = lib().size("scsfm_dvis_range_workspace_bytes", r.total, f64)
    ws = np.full(nbytes // r.buf.itemsize, np.nan, T)
    out = np.full((len(r), 2), 123.0)
    lib().call("scsfm_dvis_range", len(r), f64, _ptr(r.buf), _ptr(r.off), _ptr(r.h), _ptr(r.w), r.total, _ptr(lo),
               _ptr(hi), _ptr(t), _ptr(ws), nbytes, _ptr(out), None)
    return out


def colourise(maps, ranges, shift=0, pad=5):
    """-> pictures [H_i, W_i, 3]; every picture is written into a canvas whose rows are ``pad`` bytes longer, and the
    bytes between the rows must stay 0xAB."""
    r = maps if isinstance(maps, Ragged) else Ragged.pack(maps, shift)
    ranges = np.ascontiguousarray(ranges, np.float64)
    pitch = (3 * r.sizes[:, 1] + pad).astype(np.int32)
    size = pitch.astype(np.int64) * r.sizes[:, 0]
    ooff = (np.concatenate([[0], np.cumsum(size)[:-1]]) + 7).astype(np.int64)
    out = np.full(int(size.sum()) + 16, 0xAB, np.uint8)
    table = np.ascontiguousarray(depth_vis.MAGMA)
    lib().call("scsfm_dvis_colourise", len(r), int(r.buf.dtype == np.float64), _ptr(r.buf), _ptr(r.off), _ptr(r.h),
               _ptr(r.w), r.max_hw, _ptr(ranges), _ptr(table), _ptr(out), _ptr(ooff), _ptr(pitch), None)
    pics, seen = [], np.zeros(len(out), bool)
    for i in range(len(r)):
        H, W = r.sizes[i]
        rows = out[ooff[i]:ooff[i] + size[i]].reshape(H, pitch[i])
        pics.append(rows[:, :3 * W].reshape(H, W, 3).copy())
        mark = seen[ooff[i]:ooff[i] + size[i]].reshape(H, pitch[i])
        mark[:, :3 * W] = True
    assert (out[~seen] == 0xAB).all()
    return pics
