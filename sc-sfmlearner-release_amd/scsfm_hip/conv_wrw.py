"""The depth decoder's low-channel 3x3 convolutions with their weight gradient from libscsfm_wrw.so
(include/scsfm_wrw.h).

    conv3x3_valid(x_padded, weight) = F.conv2d(x_padded, weight)        (3x3, stride 1, no padding, no bias)

The forward is MIOpen's, unchanged.  The backward takes the input gradient from aten.convolution_backward with the
output mask [True, False, False] (MIOpen's data-gradient kernel alone; for the pairs in ROUTED_DGRAD, with
config.decoder_dgrad(), from libscsfm_dgrad.so's kernel on the same matrix instruction) and the weight gradient from the
HIP kernel,
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
# the channel counts libscsfm_dgrad.so's data gradient takes (scsfm_dgrad_conv3x3_covers; tests/test_dgrad_library.py
# compares the two)
DGRAD_COUT = (16,)
DGRAD_CIN = (16, 32)
# (Cin, Cout) whose input gradient is routed to it with config.decoder_dgrad(): those whose launch alone, at the shapes of
# configs[1], takes less than MIOpen's data-gradient op by more than the spread (profiles/decoder_dgrad_layers.txt)
ROUTED_DGRAD = {(16, 16), (32, 16)}


def covers(cin, cout):
    return int(cin) in CIN and int(cout) in COUT


def dgrad_covers(cin, cout):
    return int(cin) in DGRAD_CIN and int(cout) in DGRAD_COUT


def _plain3x3(x, m):
    """CUDA fp32 contiguous NCHW x and weight of a plain 3x3 / stride 1 / no padding / one group convolution"""
    w = m.weight
    return (x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.is_contiguous()
            and w.is_cuda and w.dtype == torch.float32 and w.is_contiguous() and tuple(w.shape[2:]) == (3, 3)
            and tuple(m.stride) == (1, 1) and tuple(m.padding) == (0, 0) and tuple(m.dilation) == (1, 1)
            and m.groups == 1 and m.padding_mode == "zeros" and x.shape[1] == w.shape[1]
            and x.shape[2] >= 3 and x.shape[3] >= 3)


def applies(x, m):
    """Does the 3x3 convolution module `m`, called on the padded `x`, take conv3x3_valid?  CUDA fp32 contiguous NCHW, a
    plain 3x3 / stride 1 / no padding / one group convolution with routed channel counts, and
    config.decoder_wrw()."""
    w = m.weight
    return bool(config.decoder_wrw() and _plain3x3(x, m) and (int(w.shape[1]), int(w.shape[0])) in ROUTED)


def applies_without_wrw(x, m):
    """Does `m`, called on the padded `x`, take conv3x3_valid(..., wrw=False) -- the input gradient from
    libscsfm_dgrad.so, the weight gradient MIOpen's?  forward_fused_bias asks where `applies` does not hold
    (SCSFM_DECODER_WRW=0), so that the input gradients of the layers in ROUTED_DGRAD, and with them every gradient
    upstream, do not depend on the weight-gradient switch."""
    w = m.weight
    return bool(config.decoder_dgrad() and _plain3x3(x, m) and (int(w.shape[1]), int(w.shape[0])) in ROUTED_DGRAD)


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


def data_grad_routed(gy, weight):
    """Does conv3x3_valid's backward take this input gradient from libscsfm_dgrad.so?  CUDA fp32 contiguous tensors, routed
    channel counts and config.decoder_dgrad()."""
    return (config.decoder_dgrad() and gy.is_cuda and gy.dtype == torch.float32 and gy.is_contiguous()
            and weight.is_cuda and weight.dtype == torch.float32 and weight.is_contiguous()
            and (int(weight.shape[1]), int(weight.shape[0])) in ROUTED_DGRAD)


def data_grad(gy, weight):
    """dx[B, Cin, H + 2, W + 2] of conv3x3_valid from the output gradient gy[B, Cout, H, W] and weight[Cout, Cin, 3, 3],
    with libscsfm_dgrad.so"""
    B, Cout, H, W = gy.shape
    Cin = weight.shape[1]
    if not (gy.is_cuda and weight.is_cuda and gy.dtype == weight.dtype == torch.float32 and gy.is_contiguous()
            and weight.is_contiguous() and tuple(weight.shape) == (Cout, Cin, 3, 3) and dgrad_covers(Cin, Cout)):
        raise ValueError(f"scsfm_hip.conv_wrw: CUDA fp32 contiguous gy[B, 16, H, W] and weight[16, 16 | 32, 3, 3] only "
                         f"(got {gy.device} {gy.dtype} {tuple(gy.shape)} and {weight.dtype} {tuple(weight.shape)})")
    dx = torch.empty((B, Cin, H + 2, W + 2), dtype=torch.float32, device=gy.device)
    _lib.get_dgrad().call("scsfm_dgrad_conv3x3_f32", B, Cin, Cout, H, W, gy.data_ptr(), weight.data_ptr(),
                          dx.data_ptr(), _stream(gy))
    return dx


class _Conv3x3Valid(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, wrw=True):
        ctx.save_for_backward(x, weight)
        ctx.wrw = wrw
        return F.conv2d(x, weight)

    @staticmethod
    def backward(ctx, gy):
        x, weight = ctx.saved_tensors
        gy = gy.contiguous()
        gx = gw = None

        def miopen(k):
            mask = [k == 0, k == 1, False]
            return torch.ops.aten.convolution_backward(gy, x, weight, None, [1, 1], [0, 0], [1, 1], False, [0, 0], 1,
                                                       mask)[k]

        if ctx.needs_input_grad[0]:  # (data_grad_routed, data_grad and weight_grad are looked up at call time)
            gx = data_grad(gy, weight) if data_grad_routed(gy, weight) else miopen(0)
        if ctx.needs_input_grad[1]:
            gw = weight_grad(x, gy) if ctx.wrw else miopen(1)
        return gx, gw, None


def conv3x3_valid(x_padded, weight, wrw=True):
    """F.conv2d(x_padded, weight) whose backward computes the weight gradient with libscsfm_wrw.so (wrw=False: MIOpen's)
    and, for the pairs in ROUTED_DGRAD with config.decoder_dgrad(), the input gradient with libscsfm_dgrad.so"""
    return _Conv3x3Valid.apply(x_padded, weight, bool(wrw))
