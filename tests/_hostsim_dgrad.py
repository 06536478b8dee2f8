"""Compiles the tail-backward kernels (sc-sfmlearner-release_amd/csrc_dgrad/*.hip), unchanged, against the host
simulator (tests/hostsim/hip/hip_runtime.h, with tests/hostsim/wrw_shim.h injected as for csrc_wrw) with g++ into
tests/hostsim/_build_dgrad/, and runs the C ABI of include/scsfm_dgrad.h on HOST pointers.  As in tests/_hostsim_decb.py
every output and the workspace are pre-filled with NaN (or with `fill`) and every array lies between two guard bands of
NaN, which `_Call.run` checks after the call.  `head_tail` at the end stands in for scsfm_hip.decoder_dgrad's on CPU
tensors.  Test infrastructure only; never loaded by the product."""
from __future__ import annotations

import ctypes
import functools
import os

import numpy as np
import torch
import torch.nn.functional as F

import _hostsim_decb as HB
from hostsim import library
from scsfm_hip._lib import DGRAD_ABI_VERSION, DGRAD_HEADER, CLib

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(ROOT, "sc-sfmlearner-release_amd", "csrc_dgrad")
HOSTSIM = os.path.join(HERE, "hostsim")
SHIM = os.path.join(HOSTSIM, "wrw_shim.h")
OUT = os.path.join(HOSTSIM, "_build_dgrad")
LIB = os.path.join(OUT, "libscsfm_dgrad_hostsim.so")
GUARD_MAX = 1 << 16


def build(force=False, src=SRC, lib=LIB):
    return library.build("dgrad", force, src, lib, shim=SHIM, dep=os.path.abspath(__file__))


@functools.lru_cache(maxsize=1)
def lib():
    return CLib(build(), DGRAD_HEADER, DGRAD_ABI_VERSION, "scsfm_dgrad_")


def ws_bytes(B, C, H, W):
    return lib().size("scsfm_dgrad_head_tail_ws_bytes", B, C, H, W)


def _ptr(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


class _Call:
    """the arrays of one call, each inside a NaN-filled buffer of its own; run() checks every band afterwards"""

    def __init__(self):
        self.bands = []

    def _place(self, shape, dtype=np.float32):
        n = int(np.prod(shape))
        g = min(n, GUARD_MAX) + 64
        buf = np.full(n + 2 * g, np.nan, dtype)
        self.bands += [buf[:g], buf[g + n:]]
        return buf[g:g + n].reshape(shape)

    def arg(self, a):
        if a is None:
            return None
        v = self._place(a.shape)
        v[...] = a
        return v

    def out(self, shape, fill, dtype=np.float32):
        v = self._place(shape, dtype)
        v[...] = fill
        return v

    def run(self, name, *args, status=0):
        rc = lib()._fn[name](*args)
        assert rc == status, f"{name} returned {rc}"
        assert all(np.isnan(b).all() for b in self.bands), f"{name} wrote outside its arrays"


def tail_bwd(q, y, g_out, w, alpha, with_bias_b=True, with_bias_head=True, fill=np.nan):
    """-> g, g_b, g_bias_b (None without), g_bias_head (None without), ws; ws is allocated (and pre-filled) also without
    a sum, to show that it stays untouched"""
    k = _Call()
    B, C, Hp, Wp = q.shape
    H, W = Hp - 2, Wp - 2
    assert g_out.shape == (B, 1, H, W) and (y is None or y.shape == g_out.shape) and w.shape == (1, C, 3, 3)
    q, y, g_out, w = k.arg(q), k.arg(y), k.arg(g_out), k.arg(w)
    n = ws_bytes(B, C, H, W)
    assert n > 0 and n % 8 == 0
    g, g_b = k.out((B, 1, H, W), fill), k.out((B, C, H, W), fill)
    ws = k.out((n // 8,), fill, np.float64)
    g_bias_b = k.out((C,), fill) if with_bias_b else None
    g_bias_head = k.out((1,), fill) if with_bias_head else None
    k.run("scsfm_dgrad_head_tail_bwd_f32", B, C, H, W, alpha, _ptr(q), _ptr(y), _ptr(g_out), _ptr(w), _ptr(g),
          _ptr(g_b), _ptr(ws), n, _ptr(g_bias_b), _ptr(g_bias_head), None)
    return g, g_b, g_bias_b, g_bias_head, ws


def conv3x3_dgrad(dy, w, fill=np.nan):
    """-> dx[B, Cin, H + 2, W + 2] from dy[B, Cout, H, W] and w[Cout, Cin, 3, 3]"""
    k = _Call()
    B, Cout, H, W = dy.shape
    Cin = w.shape[1]
    assert w.shape == (Cout, Cin, 3, 3)
    dy, w = k.arg(dy), k.arg(w)
    dx = k.out((B, Cin, H + 2, W + 2), fill)
    k.run("scsfm_dgrad_conv3x3_f32", B, Cin, Cout, H, W, _ptr(dy), _ptr(w), _ptr(dx), None)
    return dx


DATA_GRAD_CALLS = []


def data_grad(gy, weight):
    """scsfm_hip.conv_wrw.data_grad on CPU fp32 tensors, over the simulator; DATA_GRAD_CALLS lists (Cin, Cout)"""
    assert gy.dtype == torch.float32 and not gy.is_cuda and gy.dim() == 4
    DATA_GRAD_CALLS.append((int(weight.shape[1]), int(weight.shape[0])))
    return torch.from_numpy(conv3x3_dgrad(gy.detach().contiguous().numpy(), weight.detach().contiguous().numpy()).copy())


# scsfm_hip.decoder_dgrad.head_tail on CPU tensors (same saved tensors, same returns): the forward over
# tests/_hostsim_decb.py's kernels and ATen's convolution, the backward over tail_bwd above.  CALLS counts the backward
# calls.

CALLS = [0]


def _np(t):
    return t.detach().contiguous().numpy()


class _HeadTail(torch.autograd.Function):
    @staticmethod
    def forward(ctx, b, bias_b, head_weight, head_bias, alpha, beta):
        assert b.dtype == torch.float32 and not b.is_cuda and b.dim() == 4
        q = torch.from_numpy(HB.bias_elu_pad_fwd(_np(b), _np(bias_b)))
        h = F.conv2d(q, head_weight.detach())
        y, out = HB.disp_head_fwd(_np(h), _np(head_bias), float(alpha), float(beta))
        ctx.save_for_backward(q, torch.from_numpy(y), head_weight)
        ctx.alpha = float(alpha)
        return torch.from_numpy(out)

    @staticmethod
    def backward(ctx, g_out):
        from scsfm_hip import decoder_dgrad as DG
        q, y, head_weight = ctx.saved_tensors
        need_b, need_bias_b, need_w, need_bias_h = ctx.needs_input_grad[:4]
        CALLS[0] += 1
        g, g_b, g_bias_b, g_bias_h, _ = tail_bwd(_np(q), _np(y), _np(g_out), _np(head_weight), ctx.alpha, need_bias_b,
                                                 need_bias_h)
        g_w = DG._head_weight_grad(q, torch.from_numpy(g), head_weight.detach()) if need_w else None
        t = lambda a: None if a is None else torch.from_numpy(a)  # noqa: E731
        return (t(g_b) if need_b else None), t(g_bias_b), g_w, t(g_bias_h), None, None


def head_tail(b, bias_b, head_weight, head_bias, alpha, beta):
    return _HeadTail.apply(b, bias_b, head_weight, head_bias, alpha, beta)
