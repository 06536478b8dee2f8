"""Compiles the decoder kernels (sc-sfmlearner-release_amd/csrc_nets/*.hip), unchanged, against the host simulator
(tests/hostsim/hip/hip_runtime.h, plus tests/hostsim/nets_shim.h for the device library's integer min / max) with g++
into tests/hostsim/_build_nets/, and runs the C ABI of include/scsfm_nets.h on HOST pointers.  Every output is
pre-filled with NaN (or with `fill`: two runs with different fills show which entries a call left untouched), and every
array lies between two guard bands of NaN: an index that leaves its array reads NaN or is caught by `_Call.run`'s check
of the bands, where it would otherwise fault or go unnoticed.  The three autograd functions at the end stand in for
scsfm_hip.decoder's on CPU tensors.  Test infrastructure only; never loaded by the product."""
from __future__ import annotations

import ctypes
import functools
import os

import numpy as np
import torch

from hostsim import library
from scsfm_hip._lib import NETS_ABI_VERSION, NETS_HEADER, CLib

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(ROOT, "sc-sfmlearner-release_amd", "csrc_nets")
HOSTSIM = os.path.join(HERE, "hostsim")
SHIM = os.path.join(HOSTSIM, "nets_shim.h")
OUT = os.path.join(HOSTSIM, "_build_nets")
LIB = os.path.join(OUT, "libscsfm_nets_hostsim.so")


def build(force=False, src=SRC, lib=LIB):
    return library.build("nets", force, src, lib, shim=SHIM, dep=os.path.abspath(__file__))


@functools.lru_cache(maxsize=1)
def lib():
    return CLib(build(), NETS_HEADER, NETS_ABI_VERSION, "scsfm_nets_")


def _ptr(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


GUARD_MAX = 1 << 18  # elements of a guard band: the array's own size (an index up to twice too large), at most this


class _Call:
    """the arrays of one call, each inside a NaN-filled buffer of its own; run() checks every band afterwards"""

    def __init__(self):
        self.bands = []

    def _place(self, shape):
        n = int(np.prod(shape))
        g = min(n, GUARD_MAX) + 64
        buf = np.full(n + 2 * g, np.nan, np.float32)
        self.bands += [buf[:g], buf[g + n:]]
        return buf[g:g + n].reshape(shape)

    def arg(self, a):
        """a read-only argument (None stays None)"""
        if a is None:
            return None
        v = self._place(a.shape)
        v[...] = a
        return v

    def out(self, shape, fill):
        v = self._place(shape)
        v[...] = fill
        return v

    def run(self, name, *args):
        lib().call(name, *args)
        assert all(np.isnan(b).all() for b in self.bands), f"{name} wrote outside its arrays"


def pad_fwd(x, elu, fill=np.nan):
    """-> out[B, C, H+2, W+2] = R(elu ? E(x) : x)"""
    k = _Call()
    x = k.arg(x)
    B, C, H, W = x.shape
    out = k.out((B, C, H + 2, W + 2), fill)
    k.run("scsfm_nets_pad_fwd_f32", B, C, H, W, int(elu), _ptr(x), _ptr(out), None)
    return out


def pad_bwd(gp, out, elu, fill=np.nan):
    """-> g_x[B, C, H, W] from the padded gradient gp and (with elu) the forward's output"""
    k = _Call()
    gp, out = k.arg(gp), k.arg(out if elu else None)
    B, C, Hp, Wp = gp.shape
    g_x = k.out((B, C, Hp - 2, Wp - 2), fill)
    k.run("scsfm_nets_pad_bwd_f32", B, C, Hp - 2, Wp - 2, int(elu), _ptr(gp), _ptr(out), _ptr(g_x), None)
    return g_x


def up_cat_pad_fwd(a, skip, fill=np.nan):
    """-> out[B, Ca+Cs, 2H+2, 2W+2] = R(cat[U(E(a)), skip]); skip None or with no channels: Cs = 0"""
    k = _Call()
    B, Ca, H, W = a.shape
    Cs = 0 if skip is None else skip.shape[1]
    assert Cs == 0 or skip.shape == (B, Cs, 2 * H, 2 * W)
    a, skip = k.arg(a), k.arg(skip if Cs else None)
    out = k.out((B, Ca + Cs, 2 * H + 2, 2 * W + 2), fill)
    k.run("scsfm_nets_up_cat_pad_fwd_f32", B, Ca, Cs, H, W, _ptr(a), _ptr(skip), _ptr(out), None)
    return out


def up_cat_pad_bwd(gp, out, Ca, fill=np.nan):
    """-> g_a[B, Ca, H, W], g_skip[B, Cs, 2H, 2W] (None when Cs = 0) from the padded gradient and the forward's output"""
    k = _Call()
    B, Ct, Hp, Wp = gp.shape
    Cs, H, W = Ct - Ca, (Hp - 2) // 2, (Wp - 2) // 2
    assert out.shape == gp.shape and Hp == 2 * H + 2 and Wp == 2 * W + 2
    gp, out = k.arg(gp), k.arg(out)
    g_a = k.out((B, Ca, H, W), fill)
    g_skip = k.out((B, Cs, 2 * H, 2 * W), fill) if Cs else None
    k.run("scsfm_nets_up_cat_pad_bwd_f32", B, Ca, Cs, H, W, _ptr(gp), _ptr(out), _ptr(g_a), _ptr(g_skip), None)
    return g_a, g_skip


# scsfm_hip.decoder's three functions on CPU tensors (same saved tensors, same returns), over the wrappers above

def _np(t):
    return t.detach().contiguous().numpy()


class _Pad(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, elu):
        assert x.dtype == torch.float32 and not x.is_cuda and x.dim() == 4
        out = torch.from_numpy(pad_fwd(_np(x), elu))
        ctx.elu = elu
        if elu:
            ctx.save_for_backward(out)
        return out

    @staticmethod
    def backward(ctx, gp):
        out = ctx.saved_tensors[0] if ctx.elu else None
        return torch.from_numpy(pad_bwd(_np(gp), None if out is None else _np(out), ctx.elu)), None


class _UpCatPad(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, skip):
        assert a.dtype == torch.float32 and not a.is_cuda and a.dim() == 4
        out = torch.from_numpy(up_cat_pad_fwd(_np(a), None if skip is None else _np(skip)))
        ctx.save_for_backward(out)
        ctx.Ca = a.shape[1]
        return out

    @staticmethod
    def backward(ctx, gp):
        (out,) = ctx.saved_tensors
        g_a, g_skip = up_cat_pad_bwd(_np(gp), _np(out), ctx.Ca)
        return torch.from_numpy(g_a), None if g_skip is None else torch.from_numpy(g_skip)


def pad(x):
    return _Pad.apply(x, False)


def elu_pad(b):
    return _Pad.apply(b, True)


def up_cat_pad(a, skip=None):
    return _UpCatPad.apply(a, skip)
