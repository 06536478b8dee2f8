"""What the encoder's fused EVAL-mode ops (scsfm_hip.encoder_eval, libscsfm_enceval.so) are tested against, shared by the
host-simulator and the GPU tests: seeded inputs, the ATen chain they replace -- nn.BatchNorm2d(...).eval() -> + identity
-> relu (-> max_pool2d(3, 2, 1)) -- in fp64 as the yardstick and in fp32 beside it, under the contract of
tests/_encoder_ref.py

    max|fused32 - ref64| <= 2 * max|aten32 - ref64| + 4 u * max|ref64|,   u = 2^-24

per compared tensor.  The eval-mode forward is continuous in its inputs (there is no gradient whose mask could flip), so
no pre-activation has to be kept off the ReLU's kink.

The cases (make_case): channel 0 has |running_mean| = 100 sqrt(running_var) with x within a few standard deviations of
the mean (the cancellation case); channel 1 has a negative gamma; where there are at least three channels the last has
gamma = 0; one channel (1 with fewer than four channels, else 2) has running_var = 0, so eps carries it.  ``special``
plants a NaN (channel 0) and an inf (channel 1, negative gamma) in x: those entries are compared as bit patterns against
ATen, the rest under the contract."""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from _encoder_ref import U, check_contract, report  # noqa: F401  (U and report are re-exported to the tests)

EPS = 1e-5
MODES = {0: "bn", 1: "bn_relu", 2: "bn_add_relu"}
# the smallest shapes at which each path of the kernels can go wrong
SCALAR_SHAPES = [(1, 3, 2, 2), (2, 5, 3, 3), (3, 2, 5, 263), (1, 4, 7, 131)]   # H*W % 4 != 0
VECTOR_SHAPES = [(2, 3, 4, 8), (1, 2, 6, 10)]                                  # H*W % 4 == 0, the second with W % 4 != 0
TINY_PLANE = (1, 512, 8, 26)      # layer 4 at 256 x 832: four planes to a workgroup
LARGE_PLANE = (1, 64, 128, 416)   # the stem at 256 x 832: 52 chunks to a plane
BN_SHAPES = SCALAR_SHAPES + VECTOR_SHAPES + [TINY_PLANE, LARGE_PLANE]
POOL_SHAPES = [(1, 2, 1, 1), (1, 3, 5, 7), (2, 4, 6, 8), (1, 64, 32, 104)]


def make_case(shape, mode, seed, device="cpu", special=False):
    """x, identity (mode 2), gamma, beta, running_mean, running_var as fp64 tensors with fp32-representable values"""
    B, C, H, W = shape
    gen = torch.Generator(device=device).manual_seed(seed)
    kw = dict(generator=gen, dtype=torch.float64, device=device)
    rm = torch.randn(C, **kw)
    rv = 0.5 + torch.rand(C, **kw)
    rm[0] = 100.0 * rv[0].sqrt() * (1.0 if seed % 2 else -1.0)
    spread = rv.sqrt() * (0.5 + torch.rand(C, **kw))
    zero_var = None
    if C > 1:
        zero_var = 1 if C < 4 else 2
        rv[zero_var] = 0.0
        spread[zero_var] = 0.01   # invstd is 1 / sqrt(eps) = 316 there
    x = rm.view(1, C, 1, 1) + spread.view(1, C, 1, 1) * torch.randn(shape, **kw)
    gamma = torch.randn(C, **kw)
    gamma[gamma.abs() < 0.1] = 0.5
    if C > 1:
        gamma[1] = -abs(gamma[1])
    beta = 0.3 * torch.randn(C, **kw)
    if C > 2:
        gamma[C - 1] = 0.0
    identity = torch.randn(shape, **kw) if mode == 2 else None
    f = lambda t: None if t is None else t.float().double()  # noqa: E731
    x, identity, gamma, beta, rm, rv = f(x), f(identity), f(gamma), f(beta), f(rm), f(rv)
    if special:
        x[0, 0, 0, 0] = float("nan")
        x[B - 1, min(1, C - 1), H - 1, W - 1] = float("inf")
    return dict(x=x, identity=identity, gamma=gamma, beta=beta, running_mean=rm, running_var=rv, mode=mode,
                zero_var=zero_var)


def eval_bn(case, dtype, device=None):
    """nn.BatchNorm2d in eval mode holding the case's vectors"""
    C = case["x"].shape[1]
    bn = nn.BatchNorm2d(C, eps=EPS).to(device or case["x"].device, dtype)
    with torch.no_grad():
        bn.weight.copy_(case["gamma"])
        bn.bias.copy_(case["beta"])
        bn.running_mean.copy_(case["running_mean"])
        bn.running_var.copy_(case["running_var"])
    return bn.eval()


def aten_chain(case, dtype, pool=False):
    """The chain the fused op replaces, in ``dtype`` on the case's device -> dict(y[, pooled])"""
    bn = eval_bn(case, dtype)
    with torch.no_grad():
        y = bn(case["x"].to(dtype))
        if case["identity"] is not None:
            y = y + case["identity"].to(dtype)
        if case["mode"]:
            y = F.relu(y)
        out = dict(y=y)
        if pool:
            out["pooled"] = F.max_pool2d(y, 3, 2, 1)
    return out


def bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.int32)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def check_eval_contract(what, fused, aten32, ref64):
    """check_contract of tests/_encoder_ref.py; entries where the fp64 chain is not finite (a planted NaN / inf and what
    it reaches) must instead carry ATen's bit patterns"""
    fused, aten32, ref64 = dict(fused), dict(aten32), dict(ref64)
    for name in fused:
        odd = ~torch.isfinite(ref64[name]).cpu()
        if bool(odd.any()):
            got, want = bits(fused[name]), bits(aten32[name])
            odd_np = odd.numpy()
            assert np.array_equal(got[odd_np], want[odd_np]), (what, name, "NaN / inf bit patterns differ from ATen's")
            zero = lambda t: t.cpu().masked_fill(odd, 0.0)  # noqa: E731
            fused[name], aten32[name], ref64[name] = zero(fused[name]), zero(aten32[name]), zero(ref64[name])
    check_contract(what, fused, aten32, ref64)
