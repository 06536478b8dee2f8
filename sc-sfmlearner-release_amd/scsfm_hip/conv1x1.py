"""The encoders' 1x1 down-sample convolutions and the pose decoder's squeeze with their backward from libscsfm_pw.so
(include/scsfm_pw.h).

    conv1x1(x, weight, bias, stride) = F.conv2d(x, weight, bias, stride)        (1x1, stride 1 or 2, no padding)

The forward is MIOpen's, unchanged.  The backward takes the weight gradient of the triples (Cin, Cout, stride) in ROUTED
and the input gradient of those in ROUTED_DGRAD from the HIP kernels, which read x, the weight and the output gradient as
they lie (NCHW): MIOpen's paths for these memory-bound problems transpose the operands to NHWC, zero-fill the result and
transpose it back.  Everything else -- a triple that is not routed, and the bias gradient -- comes from
aten.convolution_backward with a one-hot output mask.  The node saves what the convolution's own node saves (input and
weight) and honours ctx.needs_input_grad: a frozen weight or input costs no launch.  CUDA fp32 contiguous tensors only; a
missing library is an error.  The launches go on torch's current stream, the workspace comes from torch.empty, and
nothing synchronises: graph capture is safe.  Two calls on the same tensors give the same bits.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from . import _lib, config
from .capi import _stream

# what the kernels take (scsfm_pw_covers; tests/test_pw_library.py compares the two)
CIN = (64, 128, 256, 512)
COUT = (128, 256, 512)
STRIDES = (1, 2)
# (Cin, Cout, stride) whose weight gradient is routed to the library: those whose two launches together, at the shapes of
# configs[1], take less than MIOpen's weight-gradient op by more than the larger spread (profiles/pw_layers.txt)
ROUTED = {(64, 128, 2), (128, 256, 2), (256, 512, 2), (512, 256, 1)}
# ... and whose input gradient is: stride 2 only, by the same rule
ROUTED_DGRAD = {(64, 128, 2), (128, 256, 2), (256, 512, 2)}


def covers(cin, cout, stride):
    return int(cin) in CIN and int(cout) in COUT and int(stride) in STRIDES


def dgrad_covers(cin, cout, stride):
    return covers(cin, cout, stride) and int(stride) == 2


def _triple(m):
    return int(m.weight.shape[1]), int(m.weight.shape[0]), int(m.stride[0])


def _plain1x1(x, m):
    """CUDA fp32 contiguous NCHW x and weight of a plain 1x1 / stride 1 or 2 / no padding / one group convolution"""
    w, b = m.weight, m.bias
    return (x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.is_contiguous() and x.numel() > 0
            and w.is_cuda and w.dtype == torch.float32 and w.is_contiguous() and tuple(w.shape[2:]) == (1, 1)
            and (b is None or (b.is_cuda and b.dtype == torch.float32))
            and tuple(m.stride) in ((1, 1), (2, 2)) and tuple(m.padding) == (0, 0) and tuple(m.dilation) == (1, 1)
            and m.groups == 1 and m.padding_mode == "zeros" and x.shape[1] == w.shape[1])


def applies(x, m):
    """Does the 1x1 convolution module `m`, called on `x`, take conv1x1?  CUDA fp32 contiguous NCHW, a plain 1x1
    convolution of stride 1 or 2 with a routed triple, grad mode on, and config.conv1x1_bwd()."""
    return bool(config.conv1x1_bwd() and torch.is_grad_enabled() and _plain1x1(x, m) and _triple(m) in ROUTED)


def _out_size(n, stride):
    return (n - 1) // stride + 1


def weight_grad(x, gy, stride):
    """dW[Cout, Cin, 1, 1] from the input x[B, Cin, H, W] and the output gradient gy[B, Cout, Ho, Wo]"""
    B, Cin, H, W = x.shape
    Cout = gy.shape[1]
    if not (x.is_cuda and gy.is_cuda and x.dtype == gy.dtype == torch.float32 and x.is_contiguous()
            and gy.is_contiguous() and tuple(gy.shape) == (B, Cout, _out_size(H, stride), _out_size(W, stride))):
        raise ValueError(f"scsfm_hip.conv1x1: CUDA fp32 contiguous x[B, Cin, H, W] and gy[B, Cout, Ho, Wo] only "
                         f"(got {x.device} {x.dtype} {tuple(x.shape)} and {gy.device} {gy.dtype} {tuple(gy.shape)})")
    lib = _lib.get_pw()
    n = lib.size("scsfm_pw_wrw_ws_bytes", B, Cin, Cout, H, W, stride)
    if n == 0:
        raise ValueError(f"scsfm_hip.conv1x1: no kernel for {Cin} -> {Cout} channels, stride {stride}, at {B} x {H} x {W}")
    ws = torch.empty(n // 4, dtype=torch.float32, device=x.device)
    dw = torch.empty((Cout, Cin, 1, 1), dtype=torch.float32, device=x.device)
    lib.call("scsfm_pw_wrw_f32", B, Cin, Cout, H, W, stride, x.data_ptr(), gy.data_ptr(), dw.data_ptr(), ws.data_ptr(),
             n, _stream(x))
    return dw


def data_grad(gy, weight, H, W):
    """dx[B, Cin, H, W] of the stride-2 convolution from the output gradient gy[B, Cout, Ho, Wo] and weight[Cout, Cin, 1, 1]"""
    B, Cout = gy.shape[:2]
    Cin = weight.shape[1]
    if not (gy.is_cuda and weight.is_cuda and gy.dtype == weight.dtype == torch.float32 and gy.is_contiguous()
            and weight.is_contiguous() and tuple(weight.shape) == (Cout, Cin, 1, 1) and dgrad_covers(Cin, Cout, 2)
            and tuple(gy.shape) == (B, Cout, _out_size(H, 2), _out_size(W, 2))):
        raise ValueError(f"scsfm_hip.conv1x1: CUDA fp32 contiguous gy[B, Cout, Ho, Wo] and weight[Cout, Cin, 1, 1] of a "
                         f"covered stride-2 convolution only (got {gy.device} {gy.dtype} {tuple(gy.shape)} and "
                         f"{weight.dtype} {tuple(weight.shape)} for {H} x {W})")
    dx = torch.empty((B, Cin, H, W), dtype=torch.float32, device=gy.device)
    _lib.get_pw().call("scsfm_pw_dgrad_f32", B, Cin, Cout, H, W, gy.data_ptr(), weight.data_ptr(), dx.data_ptr(),
                       _stream(gy))
    return dx


class _Conv1x1(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, stride):
        ctx.save_for_backward(x, weight)
        ctx.stride = stride
        ctx.bias_sizes = None if bias is None else [int(bias.shape[0])]
        return F.conv2d(x, weight, bias, stride)

    @staticmethod
    def backward(ctx, gy):
        x, weight = ctx.saved_tensors
        s = ctx.stride
        gy = gy.contiguous()
        triple = (int(weight.shape[1]), int(weight.shape[0]), s)
        gx = gw = gb = None

        def aten(k):
            mask = [k == 0, k == 1, k == 2]
            return torch.ops.aten.convolution_backward(gy, x, weight, ctx.bias_sizes, [s, s], [0, 0], [1, 1], False,
                                                       [0, 0], 1, mask)[k]

        if ctx.needs_input_grad[0]:  # (the sets, data_grad and weight_grad are looked up at call time)
            gx = data_grad(gy, weight, x.shape[2], x.shape[3]) if triple in ROUTED_DGRAD else aten(0)
        if ctx.needs_input_grad[1]:
            gw = weight_grad(x, gy, s) if triple in ROUTED else aten(1)
        if ctx.bias_sizes is not None and ctx.needs_input_grad[2]:
            gb = aten(2)
        return gx, gw, gb, None


def conv1x1(x, weight, bias=None, stride=1):
    """F.conv2d(x, weight, bias, stride) of a 1x1 convolution whose backward computes the weight gradient of the triples in
    ROUTED and the input gradient of those in ROUTED_DGRAD with libscsfm_pw.so"""
    return _Conv1x1.apply(x, weight, bias, int(stride))


def conv(m, x):
    """m(x) for the 1x1 convolution module m: through conv1x1 where `applies`, else the plain module call"""
    if applies(x, m):
        return conv1x1(x, m.weight, m.bias, int(m.stride[0]))
    return m(x)
