"""The depth decoder's glue with the convolutions' biases folded in: three autograd functions over libscsfm_decb.so
(include/scsfm_decb.h).

DepthDecoder.forward_fused_bias (models/DispResNet.py) calls its convolutions without their biases and hands each bias
to the kernel that reads the convolution's output anyway:

    elu_pad(b, bias)              R(E(b + bias[c]))                     (b: conv (i, 1)'s output without its bias)
    up_cat_pad(a, bias, skip)     R(cat[U(E(a + bias[c])), skip])       (a: conv (i, 0)'s)
    disp_head(x, bias, alpha, beta)   alpha * sigmoid(x + bias[c]) + beta   (x: a head's)

R: reflection pad by 1, E: ELU (alpha 1), U: 2x nearest upsampling.  The backward stores the activation gradients of
scsfm_hip.decoder bit for bit and, where the bias needs a gradient (ctx.needs_input_grad), sums the gradient it stores
per channel in fp64 in a fixed order: two runs give the same bits.  A frozen bias costs nothing.  CUDA fp32 contiguous
tensors only; a missing library is an error.  Launches go on torch's current stream, outputs and workspaces come from
torch.empty, and nothing synchronises: graph capture is safe.
"""
from __future__ import annotations

import torch

from . import _lib
from .capi import _stream
from .decoder import _check, _padded


def _check_bias(bias, C):
    if not (bias.is_cuda and bias.dtype == torch.float32 and bias.dim() == 1 and bias.shape[0] == C
            and bias.is_contiguous()):
        raise ValueError(f"scsfm_hip.decoder_bias: the bias must be a CUDA fp32 contiguous vector of {C} entries "
                         f"(got {bias.device} {bias.dtype} {tuple(bias.shape)})")


def _bias_sum_buffers(lib, like, want, B, C, H, W):
    """(ws, g_bias) for a summed gradient of shape [B, C, H, W]; (None, None) when the bias needs no gradient"""
    if not want:
        return None, None
    ws = torch.empty(lib.size("scsfm_decb_ws_bytes", B, C, H, W) // 8, dtype=torch.float64, device=like.device)
    return ws, torch.empty(C, dtype=torch.float32, device=like.device)


def _ptr(t):
    return 0 if t is None else t.data_ptr()


class _BiasEluPad(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, bias):
        _check(x)
        B, C, H, W = x.shape
        _check_bias(bias, C)
        out = _padded(x, C, H, W)
        _lib.get_decb().call("scsfm_decb_bias_elu_pad_fwd_f32", B, C, H, W, x.data_ptr(), bias.data_ptr(),
                             out.data_ptr(), _stream(x))
        ctx.save_for_backward(out)
        return out

    @staticmethod
    def backward(ctx, gp):
        gp = gp.contiguous()
        (out,) = ctx.saved_tensors
        B, C, Hp, Wp = gp.shape
        H, W = Hp - 2, Wp - 2
        lib = _lib.get_decb()
        g = torch.empty((B, C, H, W), dtype=gp.dtype, device=gp.device)
        ws, g_bias = _bias_sum_buffers(lib, gp, ctx.needs_input_grad[1], B, C, H, W)
        lib.call("scsfm_decb_bias_elu_pad_bwd_f32", B, C, H, W, gp.data_ptr(), out.data_ptr(), g.data_ptr(), _ptr(ws),
                 _ptr(g_bias), _stream(gp))
        return g, g_bias


class _BiasUpCatPad(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, bias, skip):
        _check(a, skip)
        B, Ca, H, W = a.shape
        _check_bias(bias, Ca)
        Cs = 0 if skip is None else skip.shape[1]
        if skip is not None and (skip.shape[0] != B or tuple(skip.shape[2:]) != (2 * H, 2 * W)):
            raise ValueError(f"up_cat_pad: skip {tuple(skip.shape)} does not match the upsampled {(B, Ca, 2 * H, 2 * W)}")
        out = _padded(a, Ca + Cs, 2 * H, 2 * W)
        _lib.get_decb().call("scsfm_decb_bias_up_cat_pad_fwd_f32", B, Ca, Cs, H, W, a.data_ptr(), bias.data_ptr(),
                             _ptr(skip), out.data_ptr(), _stream(a))
        ctx.save_for_backward(out)
        ctx.dims = (B, Ca, Cs, H, W)
        return out

    @staticmethod
    def backward(ctx, gp):
        gp = gp.contiguous()
        (out,) = ctx.saved_tensors
        B, Ca, Cs, H, W = ctx.dims
        lib = _lib.get_decb()
        g_a = torch.empty((B, Ca, H, W), dtype=gp.dtype, device=gp.device)
        g_skip = torch.empty((B, Cs, 2 * H, 2 * W), dtype=gp.dtype, device=gp.device) if Cs else None
        ws, g_bias = _bias_sum_buffers(lib, gp, ctx.needs_input_grad[1], B, Ca, H, W)
        lib.call("scsfm_decb_bias_up_cat_pad_bwd_f32", B, Ca, Cs, H, W, gp.data_ptr(), out.data_ptr(), g_a.data_ptr(),
                 _ptr(g_skip), _ptr(ws), _ptr(g_bias), _stream(gp))
        return g_a, g_bias, g_skip


class _DispHead(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, bias, alpha, beta):
        _check(x)
        B, C, H, W = x.shape
        _check_bias(bias, C)
        y, out = torch.empty_like(x), torch.empty_like(x)
        _lib.get_decb().call("scsfm_decb_disp_head_fwd_f32", B, C, H, W, x.data_ptr(), bias.data_ptr(), float(alpha),
                             float(beta), y.data_ptr(), out.data_ptr(), _stream(x))
        ctx.save_for_backward(y)
        ctx.alpha = float(alpha)
        return out

    @staticmethod
    def backward(ctx, g_out):
        g_out = g_out.contiguous()
        (y,) = ctx.saved_tensors
        B, C, H, W = y.shape
        lib = _lib.get_decb()
        g = torch.empty_like(y)
        ws, g_bias = _bias_sum_buffers(lib, y, ctx.needs_input_grad[1], B, C, 1, H * W)
        lib.call("scsfm_decb_disp_head_bwd_f32", B, C, H, W, ctx.alpha, g_out.data_ptr(), y.data_ptr(), g.data_ptr(),
                 _ptr(ws), _ptr(g_bias), _stream(y))
        return g, g_bias, None, None


def elu_pad(b, bias):
    """R(E(b + bias[c])) = nn.ReflectionPad2d(1)(F.elu(b + bias.view(1, -1, 1, 1)))"""
    return _BiasEluPad.apply(b, bias)


def up_cat_pad(a, bias, skip=None):
    """R(cat[U(E(a + bias[c])), skip])"""
    return _BiasUpCatPad.apply(a, bias, skip)


def disp_head(x, bias, alpha, beta):
    """alpha * torch.sigmoid(x + bias.view(1, -1, 1, 1)) + beta"""
    return _DispHead.apply(x, bias, alpha, beta)
