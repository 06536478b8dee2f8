"""Fine-tuning with frozen BatchNorm statistics (train.py --freeze-bn): the ResNet encoder's glue for modules that
``freeze`` holds in eval mode, with grad mode ON -- what scsfm_hip.encoder is to training and scsfm_hip.encoder_eval to
``no_grad`` inference.

    freeze(net, affine=False)          every nn.BatchNorm2d of ``net`` normalises with its running statistics from now on
    bn_act(x, bn)                      relu(bn(x))                (stem, a block's bn1 / bn2)
    bn_act(x, bn, identity)            relu(bn(x) + identity)     (a block's last BatchNorm)
    bn_act(x, bn, relu=False)          bn(x)                      (the down-sample branch; the models leave it to ATen)

``freeze`` swaps the class of each BatchNorm2d for ``FrozenBatchNorm2d``, a subclass whose ``train()`` leaves the module
in eval mode: ``net.train()`` at the top of an epoch, ``eval()`` for validation and the way back do not thaw it,
``isinstance``, pickling, ``copy.deepcopy`` and the state dict (names, values, strict loading) are those of
nn.BatchNorm2d, and nothing ever writes ``running_mean``, ``running_var`` or ``num_batches_tracked``.  With
``affine=True`` gamma and beta stop training as well.  The class is what the dispatch of models/resnet_encoder.py
recognises: a module that is merely in eval mode keeps the ATen chain.

The forward of ``bn_act`` is libscsfm_enceval.so's scsfm_enceval_bn_f32, so the values such a site gives while
fine-tuning are bit for bit those of validation and inference.  The backward is libscsfm_fbn.so (include/scsfm_fbn.h):
one pass that stores dx (and d_identity) and, when gamma or beta train, their gradients.  Saved for it: ``y`` where there is
a ReLU (it is alive anyway as the next convolution's input), and ``x`` only when a parameter gradient is wanted -- with
``affine=True`` no convolution output is kept alive for BatchNorm's sake.  The per-channel vectors are read from the
module in the backward.  The node is once-differentiable.

CUDA fp32 contiguous NCHW tensors only; ``qualifies`` says whether ``bn_act`` accepts a call, ``applies`` whether the
models send it here (the same, less the form without a ReLU, which measured slower than ATen's single kernel).  A
missing library is an error (no eager fallback here).  Launches go on torch's current stream, outputs and scratch are
allocated with torch.empty, and nothing synchronises.  ``SCSFM_FROZEN_TORCH=1`` makes both
false, which sends the same frozen modules down the ATen chain (the comparand of tools/bench_frozen_bn.py).
"""
from __future__ import annotations

import os

import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

from . import _lib
from .capi import _stream


class FrozenBatchNorm2d(nn.BatchNorm2d):
    """nn.BatchNorm2d that stays in eval mode: it normalises with its running statistics and never writes them.  Made by
    ``freeze`` from an existing module (same parameters, buffers and state dict)."""

    def train(self, mode=True):
        return super().train(False)


def freeze(net, affine=False):
    """Hold every nn.BatchNorm2d of ``net`` in eval mode for good; with ``affine`` also stop its gamma and beta from
    training.  -> the number of modules frozen (modules frozen before count again)."""
    n = 0
    for m in net.modules():
        if not isinstance(m, nn.BatchNorm2d):
            continue
        if type(m) not in (nn.BatchNorm2d, FrozenBatchNorm2d):
            raise TypeError(f"freeze: {type(m).__name__} is a BatchNorm2d with behaviour of its own")
        if not m.track_running_stats or m.running_mean is None or m.running_var is None:
            raise ValueError("freeze: a BatchNorm2d without running statistics has nothing to hold")
        m.__class__ = FrozenBatchNorm2d
        m.training = False
        if affine and m.affine:
            m.weight.requires_grad_(False)
            m.bias.requires_grad_(False)
        n += 1
    return n


def is_frozen(bn):
    return isinstance(bn, FrozenBatchNorm2d)


def _plain(t):
    return t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()


def enabled():
    """False under SCSFM_FROZEN_TORCH=1 (read at every call: a test or a benchmark may flip it within one process)"""
    return os.environ.get("SCSFM_FROZEN_TORCH") != "1"


def applies(x, *bns, relu=True):
    """True when the dispatch sends ``x`` (a convolution's output) through every BatchNorm2d in ``bns`` by the fused
    frozen path: ``qualifies``, and a ReLU behind the BatchNorm.  The form without one (the down-sample branch) is a
    single ATen kernel each way, so there is nothing to fuse, and the autograd node's host time made it measure slower
    than ATen, beyond both spreads, at each of the three stage shapes of configs[1] where it occurs when gamma and beta
    train (profiles/frozen_bn_bench.json: 65 against 54 us per site; 52 against 50 us, within the spreads, with them
    held): the dispatch leaves it to ATen.  ``bn_act(..., relu=False)`` itself stays available."""
    return bool(relu) and qualifies(x, *bns)


def qualifies(x, *bns):
    """True when ``bn_act`` accepts ``x`` and every BatchNorm2d in ``bns``: CUDA fp32 contiguous NCHW, grad mode on, the
    module frozen by ``freeze`` with affine parameters and running statistics."""
    if not enabled() or not torch.is_grad_enabled():
        return False
    if not (torch.is_tensor(x) and x.dim() == 4 and _plain(x) and 0 < x.numel() < 2 ** 31):
        return False
    for bn in bns:
        if not is_frozen(bn) or bn.training or not bn.affine or not bn.track_running_stats:
            return False
        vectors = (bn.weight, bn.bias, bn.running_mean, bn.running_var)
        if any(t is None for t in vectors) or not all(_plain(t) and t.numel() == x.shape[1] for t in vectors):
            return False
    return True


class _FrozenBnAct(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, identity, weight, bias, bn, mode):
        B, C, H, W = x.shape
        y = torch.empty_like(x)
        _lib.get_enceval().call("scsfm_enceval_bn_f32", B, C, H, W, mode, float(bn.eps), x.data_ptr(),
                                0 if identity is None else identity.data_ptr(), weight.data_ptr(), bias.data_ptr(),
                                bn.running_mean.data_ptr(), bn.running_var.data_ptr(), y.data_ptr(), _stream(x))
        ctx.mode, ctx.bn, ctx.shape = mode, bn, (B, C, H, W)
        ctx.params = bool(weight.requires_grad or bias.requires_grad)
        ctx.save_for_backward(*((y,) if mode else ()), *((x,) if ctx.params else ()))
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        lib = _lib.get_fbn()
        g = g.contiguous()
        saved = list(ctx.saved_tensors)
        y = saved.pop(0) if ctx.mode else None
        x = saved.pop(0) if ctx.params else None
        bn = ctx.bn
        B, C, H, W = ctx.shape
        dx = torch.empty_like(g)
        d_id = torch.empty_like(g) if ctx.mode == 2 else None
        dgamma = dbeta = ws = None
        n = 0
        if ctx.params:
            # (two tensors, not two views of one: AccumulateGrad takes a whole tensor as .grad without a copy)
            dgamma = torch.empty(C, dtype=torch.float32, device=g.device)
            dbeta = torch.empty(C, dtype=torch.float32, device=g.device)
            n = lib.size("scsfm_fbn_workspace_bytes", B, C, H, W)
            ws = torch.empty(n // 8, dtype=torch.float64, device=g.device)
        ptr = lambda t: 0 if t is None else t.data_ptr()  # noqa: E731
        lib.call("scsfm_fbn_bn_bwd_f32", B, C, H, W, ctx.mode, float(bn.eps), g.data_ptr(), ptr(x), ptr(y),
                 bn.weight.data_ptr(), bn.running_mean.data_ptr(), bn.running_var.data_ptr(), dx.data_ptr(), ptr(d_id),
                 ptr(dgamma), ptr(dbeta), ptr(ws), n, _stream(g))
        return dx, d_id, dgamma, dbeta, None, None


def bn_act(x, bn, identity=None, relu=True):
    """``bn(x)`` from the frozen module's running statistics, plus ``identity`` and through a ReLU as asked (an identity
    implies the ReLU), with a backward."""
    if not qualifies(x, bn):
        raise ValueError("scsfm_hip.encoder_frozen.bn_act: CUDA fp32 contiguous NCHW input, grad mode on and an affine "
                         "BatchNorm2d with running statistics that freeze() holds in eval mode only "
                         f"(got {x.device} {x.dtype} {tuple(x.shape)})")
    if identity is not None and not relu:
        raise ValueError("bn_act: the residual form ends in a ReLU")
    if identity is not None and (identity.shape != x.shape or not _plain(identity)):
        raise ValueError(f"bn_act: identity {tuple(identity.shape)} does not match x {tuple(x.shape)}")
    mode = 2 if identity is not None else (1 if relu else 0)
    return _FrozenBnAct.apply(x, identity, bn.weight, bn.bias, bn, mode)
