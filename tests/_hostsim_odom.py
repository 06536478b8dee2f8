"""Compiles the odometry kernels (sc-sfmlearner-release_amd/csrc_odom/*.hip), unchanged, against the host simulator
(tests/hostsim/hip/hip_runtime.h) with g++ into tests/hostsim/_build_odom/, and runs the C ABI of include/scsfm_odom.h on
HOST pointers.  Test infrastructure only; never loaded by the product."""
from __future__ import annotations

import ctypes
import functools
import os

import numpy as np

from hostsim import library
from scsfm_hip._lib import ODOM_ABI_VERSION, ODOM_HEADER, CLib

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(ROOT, "sc-sfmlearner-release_amd", "csrc_odom")
HOSTSIM = os.path.join(HERE, "hostsim")
OUT = os.path.join(HOSTSIM, "_build_odom")
LIB = os.path.join(OUT, "libscsfm_odom_hostsim.so")
ALIGN = {None: 0, "scale": 1, "scale_7dof": 2, "7dof": 3, "6dof": 4}


def build(force=False):
    return library.build("odom", force, dep=os.path.abspath(__file__))


@functools.lru_cache(maxsize=1)
def lib():
    return CLib(build(), ODOM_HEADER, ODOM_ABI_VERSION, "scsfm_odom_")


def _ptr(a):
    return ctypes.c_void_p(a.ctypes.data)


def _offsets(lens):
    lens = np.asarray(lens, np.int32)
    return np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int32), lens


def chain(vecs, rotation_mode="euler"):
    """Runs scsfm_odom_chain on the simulator for a list of [n_s, 6] arrays of one dtype -> (list of [n_s + 1, 3, 4]
    float64 global poses, list of [n_s, 3, 4] local matrices in the input precision)."""
    L = lib()
    dt = vecs[0].dtype
    off, lens = _offsets([len(v) for v in vecs])
    out_off = (off + np.arange(len(vecs))).astype(np.int32)
    S, max_len, total = len(vecs), int(lens.max()), int(lens.sum())
    vec = np.ascontiguousarray(np.concatenate([v.reshape(-1, 6) for v in vecs]), dt)
    local = np.zeros((max(total, 1), 12), dt)
    poses = np.full((total + S, 12), np.nan)
    nbytes = L.size("scsfm_odom_chain_workspace_bytes", S, max_len)
    ws = np.zeros(max(nbytes, 1), np.uint8)
    L.call("scsfm_odom_chain", S, max_len, int(dt == np.float64), int(rotation_mode == "quat"), _ptr(vec), _ptr(off),
           _ptr(lens), _ptr(out_off), _ptr(local), _ptr(poses), _ptr(ws), nbytes, None)
    return ([poses[o:o + n + 1].reshape(-1, 3, 4) for o, n in zip(out_off, lens)],
            [local[o:o + n].reshape(-1, 3, 4) for o, n in zip(off, lens)])


def evaluate(gts, preds, alignment=None):
    """Runs scsfm_odom_eval on the simulator for lists of [n_s, 12] float64 arrays -> dict(summary [S, 7],
    per_length [S, 8, 3], seg [S, max_seg, 5], n_seg [S], gt_rel, aligned (lists of [n_s, 12]))."""
    L = lib()
    off, lens = _offsets([len(g) for g in gts])
    S, max_len, total = len(gts), int(lens.max()), int(lens.sum())
    gt = np.ascontiguousarray(np.concatenate([np.reshape(g, (-1, 12)) for g in gts]), np.float64)
    pred = np.ascontiguousarray(np.concatenate([np.reshape(p, (-1, 12)) for p in preds]), np.float64)
    assert gt.shape == pred.shape
    max_seg = L.size("scsfm_odom_eval_max_segments", max_len)
    nbytes = L.size("scsfm_odom_eval_workspace_bytes", S, max_len, total)
    ws = np.zeros(nbytes, np.uint8)
    out = dict(summary=np.full((S, 7), np.nan), per_length=np.full((S, 8, 3), np.nan),
               seg=np.full((S, max_seg, 5), np.nan), n_seg=np.full(S, -1, np.int32))
    gt_rel, aligned = np.full((total, 12), np.nan), np.full((total, 12), np.nan)
    L.call("scsfm_odom_eval", S, max_len, total, ALIGN[alignment], _ptr(gt), _ptr(pred), _ptr(off), _ptr(lens), max_seg,
           _ptr(ws), nbytes, _ptr(out["summary"]), _ptr(out["per_length"]), _ptr(out["seg"]), _ptr(out["n_seg"]),
           _ptr(gt_rel), _ptr(aligned), None)
    out["gt_rel"] = [gt_rel[o:o + n] for o, n in zip(off, lens)]
    out["aligned"] = [aligned[o:o + n] for o, n in zip(off, lens)]
    return out
