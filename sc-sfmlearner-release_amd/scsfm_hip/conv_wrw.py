"""The depth decoder's low-channel 3x3 convolutions with their weight gradient from libscsfm_wrw.so
(include/scsfm_wrw.h).

    conv3x3_valid(x_padded, weight) = F.conv2d(x_padded, weight)        (3x3, stride 1, no padding, no bias)

The forward is MIOpen's, unchanged.  The backward takes the input gradient from aten.convolution_backward with the
output mask [True, False, False] (MIOpen's data-gradient kernel alone) and the weight gradient from the HIP kernel,
which reads x and the output gradient as they lie (NCHW): MIOpen's weight-gradient path for these shapes transposes
both to NHWC, zero-fills the result, adds into it with atomics and transposes it back.  The node saves what the
convolution's own node saves (input and weight) and honours ctx.needs_input_grad: a frozen weight costs nothing.
CUDA fp32 contiguous tensors only; a missing library is an error.  The launches go on torch's current stream, the
workspace comes from torch.empty, and nothing synchronises: graph capture is safe.  Two calls on the same tensors give
the same bits.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from . import _lib, config
from .capi import _stream

# the channel counts the kernel takes (scsfm_wrw_conv3x3_covers; tests/test_wrw_library.py compares the two)
COUT = (1, 16, 32)
CIN = (16, 32, 64, 96)
# (Cin, Cout) of the decoder's convolutions that are routed to it: those whose launches alone, at the shapes of
# configs[1], take less than MIOpen's weight-gradient op by more than the spread (profiles/decoder_wrw_layers.txt)
ROUTED = {(64, 32), (96, 32), (32, 16), (16, 16), (64, 1), (32, 1), (16, 1)}


def covers(cin, cout):
    return int(cin) in CIN and int(cout) in COUT


def applies(x, m):
    """Does the 3x3 convolution module `m`, called on the padded `x`, take conv3x3_valid?  CUDA fp32 contiguous NCHW, a
    plain 3x3 / stride 1 / no padding / one group convolution with routed channel counts, and
    config.decoder_wrw()."""
    w = m.weight
    return (config.decoder_wrw() and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.is_contiguous()
            and w.is_cuda and w.dtype == torch.float32 and w.is_contiguous() and tuple(w.shape[2:]) == (3, 3)
            and tuple(m.stride) == (1, 1) and tuple(m.padding) == (0, 0) and tuple(m.dilation) == (1, 1)
            and m.groups == 1 and m.padding_mode == "zeros" and x.shape[1] == w.shape[1]
            and (int(w.shape[1]), int(w.shape[0])) in ROUTED and x.shape[2] >= 3 and x.shape[3] >= 3)


def weight_grad(x, gy):
    """dW[Cout, Cin, 3, 3] of conv3x3_valid from the padded input x[B, Cin, H + 2, W + 2] and the output gradient
    gy[B, Cout, H, W]"""
    B, Cin, Hp, Wp = x.shape
    Cout, H, W = gy.shape[1], Hp - 2, Wp - 2
    if not (x.is_cuda and gy.is_cuda and x.dtype == gy.dtype == torch.float32 and x.is_contiguous()
            and gy.is_contiguous() and tuple(gy.shape) == (B, Cout, H, W)):
        raise ValueError(f"scsfm_hip.conv_wrw: CUDA fp32 contiguous x[B, Cin, H + 2, W + 2] and gy[B, Cout, H, W] only "
                         f"(got {x.device} {x.dtype} {tuple(x.shape)} and {gy.device} {gy.dtype} {tuple(gy.shape)})")
    lib = _lib.get_wrw()
    n = lib.size("scsfm_wrw_conv3x3_ws_bytes", B, Cin, Cout, H, W)
    if n == 0:
        raise ValueError(f"scsfm_hip.conv_wrw: no kernel for {Cin} -> {Cout} channels at {B} x {H} x {W}")
    ws = torch.empty(n // 4, dtype=torch.float32, device=x.device)
    dw = torch.empty((Cout, Cin, 3, 3), dtype=torch.float32, device=x.device)
    lib.call("scsfm_wrw_conv3x3_f32", B, Cin, Cout, H, W, x.data_ptr(), gy.data_ptr(), dw.data_ptr(), ws.data_ptr(), n,
             _stream(x))
    return dw


class _Conv3x3Valid(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight):
        ctx.save_for_backward(x, weight)
        return F.conv2d(x, weight)

    @staticmethod
    def backward(ctx, gy):
        x, weight = ctx.saved_tensors
        gy = gy.contiguous()
        gx = gw = None
        if ctx.needs_input_grad[0]:
            gx = torch.ops.aten.convolution_backward(gy, x, weight, None, [1, 1], [0, 0], [1, 1], False, [0, 0], 1,
                                                     [True, False, False])[0]
        if ctx.needs_input_grad[1]:
            gw = weight_grad(x, gy)
        return gx, gw


def conv3x3_valid(x_padded, weight):
    """F.conv2d(x_padded, weight) whose backward computes the weight gradient with libscsfm_wrw.so"""
    return _Conv3x3Valid.apply(x_padded, weight)
