"""Compiles the snippet kernels (sc-sfmlearner-release_amd/csrc_snip/*.hip), unchanged, against the host simulator
(tests/hostsim/hip/hip_runtime.h) with g++ into tests/hostsim/_build_snip/, and runs the C ABI of include/scsfm_snip.h on
HOST pointers.  Test infrastructure only; never loaded by the product."""
from __future__ import annotations

import ctypes
import functools
import os

import numpy as np

from hostsim import library
from scsfm_hip._lib import SNIP_ABI_VERSION, SNIP_HEADER, CLib

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(ROOT, "sc-sfmlearner-release_amd", "csrc_snip")
HOSTSIM = os.path.join(HERE, "hostsim")
OUT = os.path.join(HOSTSIM, "_build_snip")
LIB = os.path.join(OUT, "libscsfm_snip_hostsim.so")


def build(force=False):
    return library.build("snip", force, dep=os.path.abspath(__file__))


@functools.lru_cache(maxsize=1)
def lib():
    return CLib(build(), SNIP_HEADER, SNIP_ABI_VERSION, "scsfm_snip_")


def _ptr(a):
    return ctypes.c_void_p(a.ctypes.data)


def evaluate(vecs, gts, seq_len=5, rotation_mode="euler", with_gt_comp=True):
    """Runs scsfm_snip_eval on the simulator for lists of [n_s - 1, 6] arrays of one dtype and [n_s, 12] float64 arrays
    -> dict(pred [N, L, 3, 4], gt [N, L, 3, 4] or None, errors [N, 2], stats [4]).  Outputs start as NaN."""
    L = lib()
    dt = vecs[0].dtype
    lens = np.array([len(g) for g in gts], np.int32)
    assert all(len(v) == max(n - 1, 0) for v, n in zip(vecs, lens))
    counts = np.maximum(lens - seq_len + 1, 0)
    frame_off = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int32)
    snip_off = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.int32)
    S, total, n_snip = len(gts), int(lens.sum()), int(counts.sum())
    vec = np.zeros((total, 6), dt)
    for v, o in zip(vecs, frame_off):
        vec[o:o + len(v)] = v
    gt = np.ascontiguousarray(np.concatenate([np.reshape(g, (-1, 12)) for g in gts]), np.float64)
    pred = np.full((n_snip, seq_len, 12), np.nan)
    comp = np.full((n_snip, seq_len, 12), np.nan) if with_gt_comp else None
    errors, stats = np.full((n_snip, 2), np.nan), np.full(4, np.nan)
    nbytes = L.size("scsfm_snip_workspace_bytes", S, seq_len, total)
    ws = np.zeros(max(nbytes, 1), np.uint8)
    L.call("scsfm_snip_eval", S, seq_len, int(dt == np.float64), int(rotation_mode == "quat"), _ptr(vec), _ptr(gt),
           _ptr(frame_off), _ptr(lens), _ptr(snip_off), total, n_snip, _ptr(pred), _ptr(comp) if with_gt_comp else None,
           _ptr(errors), _ptr(stats), _ptr(ws), nbytes, None)
    return dict(pred=pred.reshape(n_snip, seq_len, 3, 4), gt=comp.reshape(n_snip, seq_len, 3, 4) if with_gt_comp else None,
                errors=errors, stats=stats)
