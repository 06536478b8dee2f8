"""The ResNet encoder's glue in eval mode over libscsfm_enceval.so (include/scsfm_enceval.h): what scsfm_hip.encoder is to
training, for every path that runs a trained network under ``net.eval()`` and ``torch.no_grad()``.

    bn_act(x, bn)                      relu(bn(x))                (stem, a block's bn1 / bn2)
    bn_act(x, bn, identity)            relu(bn(x) + identity)     (a block's last BatchNorm)
    bn_act(x, bn, relu=False)          bn(x)                      (the down-sample branch)
    max_pool(x)                        nn.MaxPool2d(3, 2, 1)(x)
    bn_act(x, bn, pool=True)           (f0, max_pool(f0)) with f0 = relu(bn(x)), one read of x       (the stem)

``bn`` is an ``nn.BatchNorm2d`` in eval mode: its running statistics normalise, and they, the affine parameters and the
batch counter are read, never written.  Eval-mode BatchNorm is a per-channel affine map, so every call is one launch
without scratch, and there is no backward: these are plain functions that build no autograd node, and ``applies``
demands that grad mode is off.  (Eval mode with grad enabled keeps the ATen chain; fine-tuning with frozen statistics,
train.py --freeze-bn, is scsfm_hip.encoder_frozen's, whose forward is this library's.)

CUDA fp32 contiguous NCHW tensors only; ``applies`` says whether a call qualifies, and the models choose their path with
it before calling in.  A missing library is an error (no eager fallback here).  Launches go on torch's current stream,
outputs are allocated with torch.empty, and nothing synchronises: graph capture is safe.  ``SCSFM_EVAL_TORCH=1`` makes
``applies`` / ``pool_applies`` false, which sends the models down the ATen chain (the comparand of
tools/bench_eval_encoder.py).
"""
from __future__ import annotations

import os

import torch

from . import _lib
from .capi import _stream


def _plain(t):
    return t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()


def enabled():
    """False under SCSFM_EVAL_TORCH=1 (read at every call: a test or a benchmark may flip it within one process)"""
    return os.environ.get("SCSFM_EVAL_TORCH") != "1"


def applies(x, *bns):
    """True when ``x`` (a convolution's output) and every BatchNorm2d in ``bns`` take the fused eval-mode path: CUDA fp32
    contiguous NCHW, grad mode off, the module in eval mode with affine parameters and running statistics."""
    if not enabled() or torch.is_grad_enabled():
        return False
    if not (torch.is_tensor(x) and x.dim() == 4 and _plain(x) and 0 < x.numel() < 2 ** 31):
        return False
    for bn in bns:
        if bn.training or not bn.affine or not bn.track_running_stats:
            return False
        vectors = (bn.weight, bn.bias, bn.running_mean, bn.running_var)
        if any(t is None for t in vectors) or not all(_plain(t) and t.numel() == x.shape[1] for t in vectors):
            return False
    return True


def pool_applies(x):
    return (enabled() and not torch.is_grad_enabled() and torch.is_tensor(x) and x.dim() == 4 and _plain(x) and
            0 < x.numel() < 2 ** 31)


def bn_act(x, bn, identity=None, relu=True, pool=False):
    """Eval-mode ``bn(x)``, plus ``identity`` and through a ReLU as asked (an identity implies the ReLU).  With
    ``pool=True`` (the stem: ReLU, no identity) -> ``(f0, max_pool(f0))`` from one kernel."""
    if not applies(x, bn):
        raise ValueError("scsfm_hip.encoder_eval.bn_act: CUDA fp32 contiguous NCHW input, grad mode off and an eval-mode "
                         "affine BatchNorm2d with running statistics only "
                         f"(got {x.device} {x.dtype} {tuple(x.shape)})")
    if identity is not None and not relu:
        raise ValueError("bn_act: the residual form ends in a ReLU")
    lib = _lib.get_enceval()
    B, C, H, W = x.shape
    vectors = (bn.weight.data_ptr(), bn.bias.data_ptr(), bn.running_mean.data_ptr(), bn.running_var.data_ptr())
    if pool:
        if identity is not None or not relu:
            raise ValueError("bn_act: pool=True is relu(bn(x)) followed by the max-pool, without an identity")
        f0 = torch.empty_like(x)
        pooled = torch.empty((B, C, (H - 1) // 2 + 1, (W - 1) // 2 + 1), dtype=x.dtype, device=x.device)
        lib.call("scsfm_enceval_bn_relu_pool_f32", B, C, H, W, float(bn.eps), x.data_ptr(), *vectors, f0.data_ptr(),
                 pooled.data_ptr(), _stream(x))
        return f0, pooled
    if identity is not None and (identity.shape != x.shape or not _plain(identity)):
        raise ValueError(f"bn_act: identity {tuple(identity.shape)} does not match x {tuple(x.shape)}")
    mode = 2 if identity is not None else (1 if relu else 0)
    y = torch.empty_like(x)
    lib.call("scsfm_enceval_bn_f32", B, C, H, W, mode, float(bn.eps), x.data_ptr(),
             0 if identity is None else identity.data_ptr(), *vectors, y.data_ptr(), _stream(x))
    return y


def max_pool(x):
    """nn.MaxPool2d(kernel_size=3, stride=2, padding=1)(x), forward only"""
    if not pool_applies(x):
        raise ValueError("scsfm_hip.encoder_eval.max_pool: CUDA fp32 contiguous NCHW tensors with grad mode off only "
                         f"(got {x.device} {x.dtype} {tuple(x.shape)})")
    B, C, H, W = x.shape
    out = torch.empty((B, C, (H - 1) // 2 + 1, (W - 1) // 2 + 1), dtype=x.dtype, device=x.device)
    _lib.get_enceval().call("scsfm_enceval_maxpool_f32", B, C, H, W, x.data_ptr(), out.data_ptr(), _stream(x))
    return out
