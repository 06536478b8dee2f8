"""The depth decoder's full-resolution tail with its backward from libscsfm_dgrad.so (include/scsfm_dgrad.h).

    head_tail(b, bias_b, head_weight, head_bias, alpha, beta)
        = alpha * sigmoid(conv3x3(R(E(b + bias_b[c])), head_weight) + head_bias) + beta

(b: conv (0, 1)'s output without its bias; R: reflection pad by 1, E: ELU.)  At level 0 the padded tensor Q = R(E(..))
has the disparity head as its only consumer, so the tail is one autograd node.  Its forward issues exactly the three
launches of scsfm_hip.decoder_bias.elu_pad, F.conv2d and scsfm_hip.decoder_bias.disp_head: the outputs keep their
bits.  Its backward is one streaming kernel for g (the head's pre-sigmoid gradient), the gradient of b and both bias
sums -- the gradient of Q, which MIOpen's data-gradient kernel used to write and the pad / ELU backward to read back, is
never stored -- plus the head's weight gradient from scsfm_hip.conv_wrw.weight_grad (aten.convolution_backward where
that does not apply).  The node honours ctx.needs_input_grad for all four inputs.  CUDA fp32 contiguous tensors only; a
missing library is an error.  Launches go on torch's current stream, outputs and workspaces come from torch.empty, and
nothing synchronises: graph capture is safe.  Two calls on the same tensors give the same bits.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from . import _lib, config, conv_wrw
from .capi import _stream
from .decoder import _check, _padded
from .decoder_bias import _check_bias, _ptr

# the channel counts the kernel takes (scsfm_dgrad_head_tail_covers; tests/test_dgrad_library.py compares the two)
CHANNELS = (16,)


def covers(C):
    return int(C) in CHANNELS


def _plain(t, dim):
    return t is not None and t.is_cuda and t.dtype == torch.float32 and t.dim() == dim and t.is_contiguous()


def applies(b, bias_b, head):
    """Does level 0's tail -- conv (0, 1)'s output `b`, its bias and the head's 3x3 convolution module `head` -- take
    head_tail?  CUDA fp32 contiguous tensors, a plain 3x3 / stride 1 / no padding / one group convolution from a covered
    channel count to one channel, and config.decoder_dgrad()."""
    w = head.weight
    return (config.decoder_dgrad() and _plain(b, 4) and _plain(bias_b, 1) and _plain(w, 4) and _plain(head.bias, 1)
            and covers(b.shape[1]) and tuple(w.shape) == (1, b.shape[1], 3, 3) and bias_b.shape[0] == b.shape[1]
            and tuple(head.stride) == (1, 1) and tuple(head.padding) == (0, 0) and tuple(head.dilation) == (1, 1)
            and head.groups == 1 and head.padding_mode == "zeros" and b.shape[2] >= 2 and b.shape[3] >= 2)


def tail_bwd(q, y, g_out, weight, alpha, want_bias_b=True, want_bias_head=True):
    """-> g[B, 1, H, W], g_b[B, C, H, W], g_bias_b[C] or None, g_bias_head[1] or None, from the padded q[B, C, H + 2,
    W + 2], the saved sigmoid y[B, 1, H, W] (None: g_out already is g) and the head's weight[1, C, 3, 3]"""
    B, C, Hp, Wp = q.shape
    H, W = Hp - 2, Wp - 2
    _check(q, y, g_out, weight)
    if not (tuple(g_out.shape) == (B, 1, H, W) and (y is None or y.shape == g_out.shape)
            and tuple(weight.shape) == (1, C, 3, 3)):
        raise ValueError(f"scsfm_hip.decoder_dgrad: q {tuple(q.shape)}, g_out {tuple(g_out.shape)} and weight "
                         f"{tuple(weight.shape)} do not belong together")
    lib = _lib.get_dgrad()
    n = lib.size("scsfm_dgrad_head_tail_ws_bytes", B, C, H, W)
    if n == 0:
        raise ValueError(f"scsfm_hip.decoder_dgrad: no kernel for {C} channels at {B} x {H} x {W}")
    g = torch.empty_like(g_out)
    g_b = torch.empty((B, C, H, W), dtype=q.dtype, device=q.device)
    ws = torch.empty(n // 8, dtype=torch.float64, device=q.device) if want_bias_b or want_bias_head else None
    g_bias_b = torch.empty(C, dtype=q.dtype, device=q.device) if want_bias_b else None
    g_bias_head = torch.empty(1, dtype=q.dtype, device=q.device) if want_bias_head else None
    lib.call("scsfm_dgrad_head_tail_bwd_f32", B, C, H, W, float(alpha), q.data_ptr(), _ptr(y), g_out.data_ptr(),
             weight.data_ptr(), g.data_ptr(), g_b.data_ptr(), _ptr(ws), n if ws is not None else 0, _ptr(g_bias_b),
             _ptr(g_bias_head), _stream(q))
    return g, g_b, g_bias_b, g_bias_head


def _head_weight_grad(q, g, weight):
    """the head's weight gradient: libscsfm_wrw.so's where scsfm_hip.conv_wrw routes (C, 1), else MIOpen's"""
    if config.decoder_wrw() and (int(q.shape[1]), 1) in conv_wrw.ROUTED:
        return conv_wrw.weight_grad(q, g)  # (looked up at call time)
    return torch.ops.aten.convolution_backward(g, q, weight, None, [1, 1], [0, 0], [1, 1], False, [0, 0], 1,
                                               [False, True, False])[1]


class _HeadTail(torch.autograd.Function):
    @staticmethod
    def forward(ctx, b, bias_b, head_weight, head_bias, alpha, beta):
        _check(b, head_weight)
        B, C, H, W = b.shape
        _check_bias(bias_b, C)
        _check_bias(head_bias, 1)
        decb = _lib.get_decb()
        q = _padded(b, C, H, W)
        decb.call("scsfm_decb_bias_elu_pad_fwd_f32", B, C, H, W, b.data_ptr(), bias_b.data_ptr(), q.data_ptr(),
                  _stream(b))
        h = F.conv2d(q, head_weight)
        y, out = torch.empty_like(h), torch.empty_like(h)
        decb.call("scsfm_decb_disp_head_fwd_f32", B, 1, H, W, h.data_ptr(), head_bias.data_ptr(), float(alpha),
                  float(beta), y.data_ptr(), out.data_ptr(), _stream(b))
        ctx.save_for_backward(q, y, head_weight)
        ctx.alpha = float(alpha)
        return out

    @staticmethod
    def backward(ctx, g_out):
        g_out = g_out.contiguous()
        q, y, head_weight = ctx.saved_tensors
        need_b, need_bias_b, need_w, need_bias_h = ctx.needs_input_grad[:4]
        g = g_b = g_bias_b = g_bias_h = g_w = None
        if need_b or need_bias_b:
            g, g_b, g_bias_b, g_bias_h = tail_bwd(q, y, g_out, head_weight, ctx.alpha, need_bias_b, need_bias_h)
        elif need_w or need_bias_h:
            # (a frozen conv (0, 1) behind a frozen encoder: the head's own backward alone, as decoder_bias.disp_head's)
            B, _, H, W = y.shape
            decb = _lib.get_decb()
            g = torch.empty_like(y)
            ws = None
            if need_bias_h:
                ws = torch.empty(decb.size("scsfm_decb_ws_bytes", B, 1, 1, H * W) // 8, dtype=torch.float64,
                                 device=y.device)
                g_bias_h = torch.empty(1, dtype=y.dtype, device=y.device)
            decb.call("scsfm_decb_disp_head_bwd_f32", B, 1, H, W, ctx.alpha, g_out.data_ptr(), y.data_ptr(),
                      g.data_ptr(), _ptr(ws), _ptr(g_bias_h), _stream(y))
        if need_w:
            g_w = _head_weight_grad(q, g, head_weight)
        return (g_b if need_b else None), g_bias_b, g_w, g_bias_h, None, None


def head_tail(b, bias_b, head_weight, head_bias, alpha, beta):
    """alpha * sigmoid(F.conv2d(R(E(b + bias_b[c])), head_weight) + head_bias) + beta"""
    return _HeadTail.apply(b, bias_b, head_weight, head_bias, alpha, beta)
