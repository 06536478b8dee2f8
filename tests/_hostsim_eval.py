"""Compiles the evaluation kernels (sc-sfmlearner-release_amd/csrc_eval/*.hip), unchanged, against the host simulator
(tests/hostsim/hip/hip_runtime.h) with g++ into tests/hostsim/_build_eval/, and runs the C ABI of include/scsfm_eval.h on
HOST pointers.  Test infrastructure only; never loaded by the product."""
from __future__ import annotations

import ctypes
import functools
import os

import numpy as np

from hostsim import library
from scsfm_hip._lib import EVAL_ABI_VERSION, EVAL_HEADER, CLib

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(ROOT, "sc-sfmlearner-release_amd", "csrc_eval")
HOSTSIM = os.path.join(HERE, "hostsim")
OUT = os.path.join(HOSTSIM, "_build_eval")
LIB = os.path.join(OUT, "libscsfm_eval_hostsim.so")


def build(force=False):
    return library.build("eval", force, dep=os.path.abspath(__file__))


@functools.lru_cache(maxsize=1)
def lib():
    return CLib(build(), EVAL_HEADER, EVAL_ABI_VERSION, "scsfm_eval_")


def _ptr(a):
    return ctypes.c_void_p(a.ctypes.data)


def pack(gts):
    """One buffer with every map at an offset that is a multiple of 4 elements; offsets / heights / widths."""
    hw = [g.shape[0] * g.shape[1] for g in gts]
    off = np.zeros(len(gts), np.int64)
    for i in range(1, len(gts)):
        off[i] = off[i - 1] + (hw[i - 1] + 3) // 4 * 4
    total = int(off[-1] + hw[-1])
    buf = np.zeros(total, gts[0].dtype)
    for g, o in zip(gts, off):
        buf[o:o + g.size] = g.ravel()
    return buf, off, np.array([g.shape[0] for g in gts], np.int32), np.array([g.shape[1] for g in gts], np.int32)


def evaluate(gts, pred, dataset, min_depth=1e-3, max_depth=None, buf=None):
    """Runs scsfm_eval_depth on the simulator -> dict(metrics[N,8], stats[N,3], count[N], flag[N]).  ``buf``: a
    pre-packed (buffer, offsets, heights, widths) to use instead of pack(gts)."""
    L = lib()
    max_depth = {"kitti": 80.0, "nyu": 10.0}[dataset] if max_depth is None else max_depth
    gts = [np.ascontiguousarray(g) for g in gts]
    pred = np.ascontiguousarray(pred)
    gbuf, off, gh, gw = buf if buf is not None else pack(gts)
    N, h, w = pred.shape
    pf, gf = int(pred.dtype == np.float64), int(gbuf.dtype == np.float64)
    max_hw = int((gh.astype(np.int64) * gw).max())
    total = gbuf.size
    nbytes = L.size("scsfm_eval_workspace_bytes", N, max_hw, total, pf, gf)
    ws = np.zeros(nbytes, np.uint8)
    out = dict(metrics=np.zeros((N, 8)), stats=np.zeros((N, 3)), count=np.zeros(N, np.int32),
               flag=np.zeros(N, np.int32))
    L.call("scsfm_eval_depth", N, h, w, pf, _ptr(pred), gf, _ptr(gbuf), _ptr(off), _ptr(gh), _ptr(gw), max_hw, total,
           int(dataset == "kitti"), min_depth, max_depth, _ptr(ws), nbytes, _ptr(out["metrics"]), _ptr(out["stats"]),
           _ptr(out["count"]), _ptr(out["flag"]), None)
    return out
