"""The ResNet encoder's glue as autograd functions over libscsfm_enc.so (include/scsfm_enc.h) and, for the stem's
BatchNorm / ReLU fused with its max-pool, libscsfm_stem.so (include/scsfm_stem.h).

    bn_act(x, bn)                      relu(bn(x))                (stem, a block's bn1 / bn2)
    bn_act(x, bn, identity)            relu(bn(x) + identity)     (a block's last BatchNorm)
    bn_act(x, bn, relu=False)          bn(x)                      (the down-sample branch)
    max_pool(x)                        nn.MaxPool2d(3, 2, 1)(x)
    bn_act(x, bn, pool=True)           (f0, max_pool(f0)) with f0 = relu(bn(x)), one read of x       (the stem)

``bn`` is an ``nn.BatchNorm2d`` in training mode: its batch statistics normalise, its running statistics and batch
counter are updated in place once per call (by the kernel -- no separate launches), and its parameters get their
gradients.  What a forward keeps for its backward (x, the per-channel mean / inverse standard deviation, the output in
the residual form, the pooling's one-byte argmax) are tensors of that call held by its autograd node, never module
state: the same module may run several forwards before one backward.  The module itself travels into the autograd
function as a non-tensor argument and the kernel writes its three buffers without bumping their version counters:
nothing here or in nn.BatchNorm2d saves those buffers for a backward, so no check depends on the counters.  The
backward nodes are once-differentiable (a double backward raises).

CUDA fp32 contiguous NCHW tensors only; ``applies`` says whether a call qualifies, and the models choose their path with
it before calling in.  A missing library is an error (no eager fallback here).  Launches go on torch's current stream,
outputs and scratch are allocated with torch.empty, and nothing synchronises: graph capture is safe.
"""
from __future__ import annotations

import torch
from torch.autograd.function import once_differentiable

from . import _lib
from .capi import _stream


def _plain(t):
    return t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()


def applies(x, *bns):
    """True when ``x`` (a convolution's output) and every BatchNorm2d in ``bns`` take the fused path: CUDA fp32
    contiguous NCHW with at least two entries per channel, the module in training mode with affine parameters, running
    statistics and a fixed momentum."""
    if not (torch.is_tensor(x) and x.dim() == 4 and _plain(x) and x.numel() < 2 ** 31 and
            x.shape[0] * x.shape[2] * x.shape[3] >= 2):
        return False
    for bn in bns:
        if not (bn.training and bn.affine and bn.track_running_stats and bn.momentum is not None):
            return False
        if not all(_plain(t) for t in (bn.weight, bn.bias, bn.running_mean, bn.running_var)):
            return False
        if not (bn.num_batches_tracked.is_cuda and bn.num_batches_tracked.dtype == torch.int64):
            return False
    return True


def pool_applies(x):
    return torch.is_tensor(x) and x.dim() == 4 and _plain(x) and 0 < x.numel() < 2 ** 31


def _workspace(lib, x):
    B, C, H, W = x.shape
    n = lib.size("scsfm_enc_bn_workspace_bytes", B, C, H, W)
    return torch.empty(n // 8, dtype=torch.float64, device=x.device), n


class _BnAct(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, identity, weight, bias, bn, mode):
        lib = _lib.get_enc()
        B, C, H, W = x.shape
        if identity is not None and (identity.shape != x.shape or not _plain(identity)):
            raise ValueError(f"bn_act: identity {tuple(identity.shape)} does not match x {tuple(x.shape)}")
        y = torch.empty_like(x)
        stat = torch.empty((3, C), dtype=torch.float32, device=x.device)
        ws, n = _workspace(lib, x)
        lib.call("scsfm_enc_bn_fwd_f32", B, C, H, W, mode, float(bn.eps), float(bn.momentum), x.data_ptr(),
                 0 if identity is None else identity.data_ptr(), weight.data_ptr(), bias.data_ptr(), y.data_ptr(),
                 stat.data_ptr(), bn.running_mean.data_ptr(), bn.running_var.data_ptr(),
                 bn.num_batches_tracked.data_ptr(), ws.data_ptr(), n, _stream(x))
        ctx.mode = mode
        ctx.save_for_backward(x, weight, bias, stat, *((y,) if mode == 2 else ()))
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        lib = _lib.get_enc()
        g = g.contiguous()
        x, weight, bias, stat = ctx.saved_tensors[:4]
        y = ctx.saved_tensors[4] if ctx.mode == 2 else None
        B, C, H, W = x.shape
        dx = torch.empty_like(x)
        d_id = torch.empty_like(x) if ctx.mode == 2 else None
        # (two tensors, not two views of one: AccumulateGrad takes a whole tensor as .grad without a copy)
        dgamma = torch.empty(C, dtype=torch.float32, device=x.device)
        dbeta = torch.empty(C, dtype=torch.float32, device=x.device)
        ws, n = _workspace(lib, x)
        lib.call("scsfm_enc_bn_bwd_f32", B, C, H, W, ctx.mode, g.data_ptr(), x.data_ptr(),
                 0 if y is None else y.data_ptr(), weight.data_ptr(), bias.data_ptr(), stat.data_ptr(), dx.data_ptr(),
                 0 if d_id is None else d_id.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(), ws.data_ptr(), n,
                 _stream(x))
        return dx, d_id, dgamma, dbeta, None, None


class _MaxPool(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        B, C, H, W = x.shape
        PH, PW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        out = torch.empty((B, C, PH, PW), dtype=x.dtype, device=x.device)
        arg = torch.empty((B, C, PH, PW), dtype=torch.uint8, device=x.device)
        _lib.get_enc().call("scsfm_enc_maxpool_fwd_f32", B, C, H, W, x.data_ptr(), out.data_ptr(), arg.data_ptr(),
                            _stream(x))
        ctx.save_for_backward(arg)
        ctx.shape = (B, C, H, W)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        g = g.contiguous()
        (arg,) = ctx.saved_tensors
        B, C, H, W = ctx.shape
        dx = torch.empty((B, C, H, W), dtype=g.dtype, device=g.device)
        _lib.get_enc().call("scsfm_enc_maxpool_bwd_f32", B, C, H, W, g.data_ptr(), arg.data_ptr(), dx.data_ptr(),
                            _stream(g))
        return dx


class _BnReluPool(torch.autograd.Function):
    """(f0, pooled) = (relu(bn(x)), max_pool(f0)).  A gradient that does not arrive stays None (the pose encoder's f0
    has no reader): the backward then runs the kernel variant that reads nothing for it."""

    @staticmethod
    def forward(ctx, x, weight, bias, bn):
        lib = _lib.get_stem()
        B, C, H, W = x.shape
        PH, PW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        f0 = torch.empty_like(x)
        out = torch.empty((B, C, PH, PW), dtype=x.dtype, device=x.device)
        arg = torch.empty((B, C, PH, PW), dtype=torch.uint8, device=x.device)
        stat = torch.empty((3, C), dtype=torch.float32, device=x.device)
        n = lib.size("scsfm_stem_workspace_bytes", B, C, H, W)
        ws = torch.empty(n // 8, dtype=torch.float64, device=x.device)
        lib.call("scsfm_stem_fwd_f32", B, C, H, W, float(bn.eps), float(bn.momentum), x.data_ptr(), weight.data_ptr(),
                 bias.data_ptr(), f0.data_ptr(), out.data_ptr(), arg.data_ptr(), stat.data_ptr(),
                 bn.running_mean.data_ptr(), bn.running_var.data_ptr(), bn.num_batches_tracked.data_ptr(),
                 ws.data_ptr(), n, _stream(x))
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(x, weight, bias, stat, arg)
        return f0, out

    @staticmethod
    @once_differentiable
    def backward(ctx, g_f0, g_pool):
        if g_f0 is None and g_pool is None:
            return None, None, None, None
        x, weight, bias, stat, arg = ctx.saved_tensors
        B, C, H, W = x.shape
        dx = torch.empty_like(x)
        dgamma = torch.empty(C, dtype=torch.float32, device=x.device)
        dbeta = torch.empty(C, dtype=torch.float32, device=x.device)
        if g_f0 is not None:
            g_f0 = g_f0.contiguous()
        if g_pool is None:
            # nothing read the pooled map: what is left is the backward of relu(bn(x)) alone
            lib = _lib.get_enc()
            ws, n = _workspace(lib, x)
            lib.call("scsfm_enc_bn_bwd_f32", B, C, H, W, 1, g_f0.data_ptr(), x.data_ptr(), 0, weight.data_ptr(),
                     bias.data_ptr(), stat.data_ptr(), dx.data_ptr(), 0, dgamma.data_ptr(), dbeta.data_ptr(),
                     ws.data_ptr(), n, _stream(x))
            return dx, dgamma, dbeta, None
        lib = _lib.get_stem()
        g_pool = g_pool.contiguous()
        n = lib.size("scsfm_stem_workspace_bytes", B, C, H, W)
        ws = torch.empty(n // 8, dtype=torch.float64, device=x.device)
        lib.call("scsfm_stem_bwd_f32", B, C, H, W, g_pool.data_ptr(), 0 if g_f0 is None else g_f0.data_ptr(),
                 arg.data_ptr(), x.data_ptr(), weight.data_ptr(), bias.data_ptr(), stat.data_ptr(), dx.data_ptr(),
                 dgamma.data_ptr(), dbeta.data_ptr(), ws.data_ptr(), n, _stream(x))
        return dx, dgamma, dbeta, None


def bn_act(x, bn, identity=None, relu=True, pool=False):
    """Train-mode ``bn(x)``, plus ``identity`` and through a ReLU as asked (an identity implies the ReLU).  With
    ``pool=True`` (the stem: ReLU, no identity) -> ``(f0, max_pool(f0))`` from one fused forward and backward."""
    if not applies(x, bn):
        raise ValueError("scsfm_hip.encoder.bn_act: CUDA fp32 contiguous NCHW input and a training-mode affine "
                         f"BatchNorm2d with running statistics only (got {x.device} {x.dtype} {tuple(x.shape)})")
    if identity is not None and not relu:
        raise ValueError("bn_act: the residual form ends in a ReLU")
    if pool:
        if identity is not None or not relu:
            raise ValueError("bn_act: pool=True is relu(bn(x)) followed by the max-pool, without an identity")
        return _BnReluPool.apply(x, bn.weight, bn.bias, bn)
    mode = 2 if identity is not None else (1 if relu else 0)
    return _BnAct.apply(x, identity, bn.weight, bn.bias, bn, mode)


def max_pool(x):
    """nn.MaxPool2d(kernel_size=3, stride=2, padding=1)(x) with a one-byte argmax for the backward"""
    if not pool_applies(x):
        raise ValueError("scsfm_hip.encoder.max_pool: CUDA fp32 contiguous NCHW tensors only "
                         f"(got {x.device} {x.dtype} {tuple(x.shape)})")
    return _MaxPool.apply(x)
