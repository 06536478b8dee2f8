"""Compiles the decoder-bias kernels (sc-sfmlearner-release_amd/csrc_decb/*.hip), unchanged, against the host simulator
(tests/hostsim/hip/hip_runtime.h) with g++ into tests/hostsim/_build_decb/, and runs the C ABI of include/scsfm_decb.h on
HOST pointers.  As in tests/_hostsim_nets.py every output (and the workspace) is pre-filled with NaN bytes (or with
`fill`) and every array lies between two guard bands of NaN, which `_Call.run` checks after the call.  The three
autograd functions at the end stand in for scsfm_hip.decoder_bias's on CPU tensors.  Test infrastructure only; never
loaded by the product."""
from __future__ import annotations

import ctypes
import functools
import os

import numpy as np
import torch

from hostsim import library
from scsfm_hip._lib import DECB_ABI_VERSION, DECB_HEADER, CLib

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(ROOT, "sc-sfmlearner-release_amd", "csrc_decb")
HOSTSIM = os.path.join(HERE, "hostsim")
OUT = os.path.join(HOSTSIM, "_build_decb")
LIB = os.path.join(OUT, "libscsfm_decb_hostsim.so")
GUARD_MAX = 1 << 18


def build(force=False, src=SRC, lib=LIB):
    return library.build("decb", force, src, lib, dep=os.path.abspath(__file__))


@functools.lru_cache(maxsize=1)
def lib():
    return CLib(build(), DECB_HEADER, DECB_ABI_VERSION, "scsfm_decb_")


def ws_bytes(B, C, H, W):
    return lib().size("scsfm_decb_ws_bytes", B, C, H, W)


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


def _sum_buffers(k, with_bias, B, C, H, W, fill):
    """(ws, g_bias); ws is allocated (and pre-filled) also without a bias sum, to show that it stays untouched"""
    ws = k.out((ws_bytes(B, C, H, W) // 8,), fill, np.float64)
    return ws, (k.out((C,), fill) if with_bias else None)


def bias_elu_pad_fwd(x, bias, fill=np.nan):
    k = _Call()
    x, bias = k.arg(x), k.arg(bias)
    B, C, H, W = x.shape
    out = k.out((B, C, H + 2, W + 2), fill)
    k.run("scsfm_decb_bias_elu_pad_fwd_f32", B, C, H, W, _ptr(x), _ptr(bias), _ptr(out), None)
    return out


def bias_elu_pad_bwd(gp, out, with_bias=True, fill=np.nan):
    """-> g_x, g_bias (None without), ws"""
    k = _Call()
    gp, out = k.arg(gp), k.arg(out)
    B, C, Hp, Wp = gp.shape
    g_x = k.out((B, C, Hp - 2, Wp - 2), fill)
    ws, g_bias = _sum_buffers(k, with_bias, B, C, Hp - 2, Wp - 2, fill)
    k.run("scsfm_decb_bias_elu_pad_bwd_f32", B, C, Hp - 2, Wp - 2, _ptr(gp), _ptr(out), _ptr(g_x), _ptr(ws),
          _ptr(g_bias), None)
    return g_x, g_bias, ws


def bias_up_cat_pad_fwd(a, bias, skip, fill=np.nan):
    k = _Call()
    B, Ca, H, W = a.shape
    Cs = 0 if skip is None else skip.shape[1]
    assert Cs == 0 or skip.shape == (B, Cs, 2 * H, 2 * W)
    a, bias, skip = k.arg(a), k.arg(bias), k.arg(skip if Cs else None)
    out = k.out((B, Ca + Cs, 2 * H + 2, 2 * W + 2), fill)
    k.run("scsfm_decb_bias_up_cat_pad_fwd_f32", B, Ca, Cs, H, W, _ptr(a), _ptr(bias), _ptr(skip), _ptr(out), None)
    return out


def bias_up_cat_pad_bwd(gp, out, Ca, with_bias=True, fill=np.nan):
    """-> g_a, g_skip (None when Cs = 0), g_bias (None without), ws"""
    k = _Call()
    B, Ct, Hp, Wp = gp.shape
    Cs, H, W = Ct - Ca, (Hp - 2) // 2, (Wp - 2) // 2
    assert out.shape == gp.shape and Hp == 2 * H + 2 and Wp == 2 * W + 2
    gp, out = k.arg(gp), k.arg(out)
    g_a = k.out((B, Ca, H, W), fill)
    g_skip = k.out((B, Cs, 2 * H, 2 * W), fill) if Cs else None
    ws, g_bias = _sum_buffers(k, with_bias, B, Ca, H, W, fill)
    k.run("scsfm_decb_bias_up_cat_pad_bwd_f32", B, Ca, Cs, H, W, _ptr(gp), _ptr(out), _ptr(g_a), _ptr(g_skip), _ptr(ws),
          _ptr(g_bias), None)
    return g_a, g_skip, g_bias, ws


def disp_head_fwd(x, bias, alpha, beta, fill=np.nan):
    """-> y, out"""
    k = _Call()
    x, bias = k.arg(x), k.arg(bias)
    B, C, H, W = x.shape
    y, out = k.out(x.shape, fill), k.out(x.shape, fill)
    k.run("scsfm_decb_disp_head_fwd_f32", B, C, H, W, _ptr(x), _ptr(bias), alpha, beta, _ptr(y), _ptr(out), None)
    return y, out


def disp_head_bwd(g_out, y, alpha, with_bias=True, fill=np.nan):
    """-> g_x, g_bias (None without), ws"""
    k = _Call()
    g_out, y = k.arg(g_out), k.arg(y)
    B, C, H, W = y.shape
    g_x = k.out(y.shape, fill)
    ws, g_bias = _sum_buffers(k, with_bias, B, C, 1, H * W, fill)
    k.run("scsfm_decb_disp_head_bwd_f32", B, C, H, W, alpha, _ptr(g_out), _ptr(y), _ptr(g_x), _ptr(ws), _ptr(g_bias),
          None)
    return g_x, g_bias, ws


# scsfm_hip.decoder_bias's three functions on CPU tensors (same saved tensors, same returns), over the wrappers above.
# REDUCTIONS counts the bias sums that ran.

REDUCTIONS = [0]


def _np(t):
    return t.detach().contiguous().numpy()


def _bias_grad(g_bias):
    if g_bias is None:
        return None
    REDUCTIONS[0] += 1
    return torch.from_numpy(g_bias)


class _BiasEluPad(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, bias):
        assert x.dtype == torch.float32 and not x.is_cuda and x.dim() == 4
        out = torch.from_numpy(bias_elu_pad_fwd(_np(x), _np(bias)))
        ctx.save_for_backward(out)
        return out

    @staticmethod
    def backward(ctx, gp):
        (out,) = ctx.saved_tensors
        g_x, g_bias, _ = bias_elu_pad_bwd(_np(gp), _np(out), ctx.needs_input_grad[1])
        return torch.from_numpy(g_x), _bias_grad(g_bias)


class _BiasUpCatPad(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, bias, skip):
        assert a.dtype == torch.float32 and not a.is_cuda and a.dim() == 4
        out = torch.from_numpy(bias_up_cat_pad_fwd(_np(a), _np(bias), None if skip is None else _np(skip)))
        ctx.save_for_backward(out)
        ctx.Ca = a.shape[1]
        return out

    @staticmethod
    def backward(ctx, gp):
        (out,) = ctx.saved_tensors
        g_a, g_skip, g_bias, _ = bias_up_cat_pad_bwd(_np(gp), _np(out), ctx.Ca, ctx.needs_input_grad[1])
        return torch.from_numpy(g_a), _bias_grad(g_bias), None if g_skip is None else torch.from_numpy(g_skip)


class _DispHead(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, bias, alpha, beta):
        assert x.dtype == torch.float32 and not x.is_cuda and x.dim() == 4
        y, out = disp_head_fwd(_np(x), _np(bias), float(alpha), float(beta))
        ctx.save_for_backward(torch.from_numpy(y))
        ctx.alpha = float(alpha)
        return torch.from_numpy(out)

    @staticmethod
    def backward(ctx, g_out):
        (y,) = ctx.saved_tensors
        g_x, g_bias, _ = disp_head_bwd(_np(g_out), _np(y), ctx.alpha, ctx.needs_input_grad[1])
        return torch.from_numpy(g_x), _bias_grad(g_bias), None, None


def elu_pad(b, bias):
    return _BiasEluPad.apply(b, bias)


def up_cat_pad(a, bias, skip=None):
    return _BiasUpCatPad.apply(a, bias, skip)


def disp_head(x, bias, alpha, beta):
    return _DispHead.apply(x, bias, alpha, beta)
