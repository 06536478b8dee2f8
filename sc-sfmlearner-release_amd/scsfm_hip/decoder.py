"""The depth decoder's glue as three autograd functions over libscsfm_nets.so (include/scsfm_nets.h).

Each one replaces the ATen chain between two of DepthDecoder's convolutions (models/DispResNet.py) by one kernel
forward and one backward, and produces the same padded tensor that chain hands the convolution:

    pad(x)                  R(x)                            (the input of conv (4, 0))
    elu_pad(b)              R(E(b))                         (b: conv (i, 1)'s output; feeds conv (i-1, 0) and head i)
    up_cat_pad(a, skip)     R(cat[U(E(a)), skip])           (a: conv (i, 0)'s output; skip None at level 0)

R: reflection pad by 1, E: ELU (alpha 1), U: 2x nearest upsampling.  CUDA fp32 contiguous NCHW tensors only; a missing
library is an error (there is no eager fallback here -- the model chooses its path before calling in).  Launches go on
torch's current stream, outputs are allocated with torch.empty, and nothing synchronises: graph capture is safe.

The backward of elu_pad / up_cat_pad reads the ELU result from the interior of its own saved output, which the
convolution saves anyway.  When both consumers of an elu_pad output backpropagate (num_scales > 1), autograd adds their
two padded gradients before the fold, where ATen's chain folds each and adds the results: the border sums are
reassociated (within an ulp of the sum's terms).  With one scale (the training default) only one gradient arrives.
"""
from __future__ import annotations

import torch

from . import _lib
from .capi import _stream


def _check(*ts):
    for t in ts:
        if t is None:
            continue
        if not (t.is_cuda and t.dtype == torch.float32 and t.dim() == 4 and t.is_contiguous()):
            raise ValueError("scsfm_hip.decoder: CUDA fp32 contiguous NCHW tensors only "
                             f"(got {t.device} {t.dtype} {tuple(t.shape)}, contiguous={t.is_contiguous()})")


def _padded(t, C, H, W):
    return torch.empty((t.shape[0], C, H + 2, W + 2), dtype=t.dtype, device=t.device)


class _Pad(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, elu):
        _check(x)
        B, C, H, W = x.shape
        out = _padded(x, C, H, W)
        _lib.get_nets().call("scsfm_nets_pad_fwd_f32", B, C, H, W, int(elu), x.data_ptr(), out.data_ptr(), _stream(x))
        ctx.elu = elu
        if elu:
            ctx.save_for_backward(out)
        return out

    @staticmethod
    def backward(ctx, gp):
        gp = gp.contiguous()
        B, C, Hp, Wp = gp.shape
        out = ctx.saved_tensors[0] if ctx.elu else None
        g = torch.empty((B, C, Hp - 2, Wp - 2), dtype=gp.dtype, device=gp.device)
        _lib.get_nets().call("scsfm_nets_pad_bwd_f32", B, C, Hp - 2, Wp - 2, int(ctx.elu), gp.data_ptr(),
                             0 if out is None else out.data_ptr(), g.data_ptr(), _stream(gp))
        return g, None


class _UpCatPad(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, skip):
        _check(a, skip)
        B, Ca, H, W = a.shape
        Cs = 0 if skip is None else skip.shape[1]
        if skip is not None and (skip.shape[0] != B or tuple(skip.shape[2:]) != (2 * H, 2 * W)):
            raise ValueError(f"up_cat_pad: skip {tuple(skip.shape)} does not match the upsampled {(B, Ca, 2 * H, 2 * W)}")
        out = _padded(a, Ca + Cs, 2 * H, 2 * W)
        _lib.get_nets().call("scsfm_nets_up_cat_pad_fwd_f32", B, Ca, Cs, H, W, a.data_ptr(),
                             0 if skip is None else skip.data_ptr(), out.data_ptr(), _stream(a))
        ctx.save_for_backward(out)
        ctx.dims = (B, Ca, Cs, H, W)
        return out

    @staticmethod
    def backward(ctx, gp):
        gp = gp.contiguous()
        (out,) = ctx.saved_tensors
        B, Ca, Cs, H, W = ctx.dims
        g_a = torch.empty((B, Ca, H, W), dtype=gp.dtype, device=gp.device)
        g_skip = torch.empty((B, Cs, 2 * H, 2 * W), dtype=gp.dtype, device=gp.device) if Cs else None
        _lib.get_nets().call("scsfm_nets_up_cat_pad_bwd_f32", B, Ca, Cs, H, W, gp.data_ptr(), out.data_ptr(),
                             g_a.data_ptr(), 0 if g_skip is None else g_skip.data_ptr(), _stream(gp))
        return g_a, g_skip


def pad(x):
    """R(x) = nn.ReflectionPad2d(1)(x)"""
    return _Pad.apply(x, False)


def elu_pad(b):
    """R(E(b)) = nn.ReflectionPad2d(1)(F.elu(b))"""
    return _Pad.apply(b, True)


def up_cat_pad(a, skip=None):
    """R(cat[U(E(a)), skip]) = nn.ReflectionPad2d(1)(torch.cat([F.interpolate(F.elu(a), scale_factor=2), skip], 1))"""
    return _UpCatPad.apply(a, skip)
