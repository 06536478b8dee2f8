"""Compiles the frozen-statistics BatchNorm backward (sc-sfmlearner-release_amd/csrc_fbn/*.hip), unchanged, against the
host simulator (tests/hostsim/hip/hip_runtime.h) with g++ into tests/hostsim/_build_fbn/, and runs the C ABI of
include/scsfm_fbn.h on HOST pointers.  Every buffer handed to the library starts on a 64-byte boundary (so the shape alone
decides between the 16-byte and the scalar path) unless ``misalign`` moves the upstream gradient 4 bytes on; every output
lies between two guard bands of a sentinel bit pattern, is pre-filled with it, and the bands are checked after the call.
The workspace is pre-filled with the sentinel too -- a NaN, so a slot that is read before it is written shows in the sums
-- and has guard bands of its own.  Test infrastructure only; never loaded by the product."""
from __future__ import annotations

import functools
import os

import numpy as np

from _hostsim_enceval import SENTINEL, _aligned, _in, _Out, _ptr
from hostsim import library
from scsfm_hip._lib import FBN_ABI_VERSION, FBN_HEADER, CLib

WS_SENTINEL = 0x7FF8DEAD7FC0DEAD   # a double NaN no kernel computes


def build(force=False):
    return library.build("fbn", force, dep=os.path.abspath(__file__))


@functools.lru_cache(maxsize=1)
def lib():
    return CLib(build(), FBN_HEADER, FBN_ABI_VERSION, "scsfm_fbn_")


def workspace_bytes(shape):
    return lib().size("scsfm_fbn_workspace_bytes", *shape)


def _off_by_four(a):
    """a copy of ``a`` that starts 4 bytes past a 64-byte boundary"""
    raw, view = _aligned((a.size + 1,))
    out = view[1:].reshape(a.shape)
    out[...] = a
    assert out.ctypes.data % 16 == 4
    return out


def bn_bwd(g, x, y, gamma, running_mean, running_var, mode, eps, params=True, misalign=False, spare_ws=False):
    """-> dict(dx[, d_identity][, dgamma, dbeta]).  The per-channel vectors are handed over as they are (float32 arrays:
    the test checks they stay unchanged).  ``params=False``: the no-parameter form (dgamma = dbeta = x = NULL);
    ``spare_ws`` hands it a workspace all the same, which must come back untouched."""
    shape = g.shape
    B, C, H, W = shape
    g = _off_by_four(g) if misalign else _in(g)
    x, y = _in(x) if params else None, _in(y) if mode else None
    dx = _Out(shape)
    d_id = _Out(shape) if mode == 2 else None
    dgamma, dbeta = (_Out((C,)), _Out((C,))) if params else (None, None)
    ws, n = None, 0
    if params or spare_ws:
        n = workspace_bytes(shape)
        assert n > 0 and n % 16 == 0
        ws = _Out((n // 4,))
        ws.view.view(np.int64)[...] = WS_SENTINEL
    lib().call("scsfm_fbn_bn_bwd_f32", B, C, H, W, mode, eps, _ptr(g), _ptr(x), _ptr(y), _ptr(gamma), _ptr(running_mean),
               _ptr(running_var), _ptr(dx.view), None if d_id is None else _ptr(d_id.view),
               None if dgamma is None else _ptr(dgamma.view), None if dbeta is None else _ptr(dbeta.view),
               None if ws is None else _ptr(ws.view), n, None)
    out = dict(dx=dx.finish("dx"))
    if d_id is not None:
        out["d_identity"] = d_id.finish("d_identity")
    if params:
        out["dgamma"], out["dbeta"] = dgamma.finish("dgamma"), dbeta.finish("dbeta")
    if ws is not None:
        bits = ws.raw.view(np.int32)
        assert np.all(bits[:ws.lo] == SENTINEL) and np.all(bits[ws.lo + ws.view.size:] == SENTINEL), \
            "ws: a guard band was written"
        if not params:
            assert np.all(ws.view.view(np.int64) == WS_SENTINEL), "the no-parameter form touched the workspace"
    return out
