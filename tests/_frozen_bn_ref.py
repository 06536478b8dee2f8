"""What the frozen-statistics BatchNorm ops (scsfm_hip.encoder_frozen, libscsfm_fbn.so) are tested against, shared by the
host-simulator and the GPU tests: seeded inputs, the ATen chain they replace -- nn.BatchNorm2d(...).eval() -> + identity
-> relu, with grad -- in fp64 as the yardstick and in fp32 beside it, under the contract of tests/_encoder_ref.py

    max|fused32 - ref64| <= 2 * max|aten32 - ref64| + 4 u * max|ref64|,   u = 2^-24

per compared tensor (dx, d_identity, dgamma, dbeta).

The cases are tests/_encoder_eval_ref.py's (the cancellation channel, a negative and a zero gamma, a channel with
running_var = 0) plus an upstream gradient, kept off the ReLU's kink as tests/_encoder_ref.py explains: every
pre-activation of the fp64 chain is exactly 0 -- the channel with gamma = 0, whose beta is 0 here as well where nothing is
added behind it -- or at least 1e-3 away from 0; entries that are not are nudged (x along gamma * invstd, or the identity)
until they are.

``special`` plants a NaN in x (so y is a NaN there and the gradient passes), and an inf and a NaN in the upstream
gradient.  Entries of dx and d_identity that are not finite in the fp64 chain are compared with ATen's as bit patterns;
a sum that is not finite has to be a NaN where ATen's is one and equal to ATen's otherwise."""
import numpy as np
import torch
import torch.nn.functional as F

import _encoder_eval_ref as EV
from _encoder_ref import U, check_contract, report  # noqa: F401  (re-exported to the tests)

EPS = EV.EPS
MODES = EV.MODES
KINK = 1e-3
SCALAR_SHAPES = [(1, 3, 2, 2), (2, 5, 3, 3), (3, 2, 5, 263), (1, 4, 7, 131)]   # small and odd planes; the third: several tasks, a tail
VECTOR_SHAPES = [(2, 3, 4, 8), (1, 2, 6, 10), (3, 2, 33, 32)]                  # H*W % 4 == 0; W % 4 != 0; a task + 32 floats
TINY_PLANES = (2, 512, 8, 26)     # layer 4 at 256 x 832: four planes to a workgroup, B slots per channel
STEM_PLANE = (1, 64, 128, 416)    # the stem at 256 x 832
SHAPES = SCALAR_SHAPES + VECTOR_SHAPES + [TINY_PLANES]


def kernel_constants():
    """kWave, kThreads, kUnroll, kMaxBlocks as csrc_fbn/scsfm_frozen_bn.hip defines them"""
    import os
    import re
    src = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "sc-sfmlearner-release_amd",
                       "csrc_fbn", "scsfm_frozen_bn.hip")
    with open(src) as f:
        text = f.read()
    return tuple(int(re.search(r"constexpr int %s = (\d+);" % name, text).group(1))
                 for name in ("kWave", "kThreads", "kUnroll", "kMaxBlocks"))


def tasks(shape, aligned=True):
    """-> (tasks, waves of the largest grid, vec): the work split of the source, in Python"""
    wave, threads, unroll, max_blocks = kernel_constants()
    B, C, H, W = shape
    vec = (H * W) % 4 == 0 and aligned
    per = H * W // 4 if vec else H * W
    return B * C * -(-per // (unroll * wave)), max_blocks * (threads // wave), vec


def _preactivation(case):
    v = F.batch_norm(case["x"], case["running_mean"], case["running_var"], case["gamma"], case["beta"], False, 0.0, EPS)
    return v if case["identity"] is None else v + case["identity"]


def make_case(shape, mode, seed, device="cpu", special=False):
    """_encoder_eval_ref.make_case plus ``g``, off the kink (module docstring); fp64 tensors with fp32-representable
    values"""
    case = EV.make_case(shape, mode, seed, device)
    B, C, H, W = shape
    gen = torch.Generator(device=device).manual_seed(seed + 7919)
    case["g"] = torch.randn(shape, generator=gen, dtype=torch.float64, device=device).float().double()
    if mode:
        zero_ch = C - 1 if C > 2 else None
        if zero_ch is not None and mode == 1:
            case["beta"][zero_ch] = 0.0   # (gamma is 0 there: every evaluation yields exactly 0 and drops the gradient)
        for _ in range(6):
            v = _preactivation(case)
            near = (v.abs() < KINK) & (v != 0)
            if not bool(near.any()):
                break
            if mode == 2:
                case["identity"] = torch.where(near, case["identity"] + 0.01, case["identity"]).float().double()
            else:
                # (a step that moves the pre-activation by 4e-3: dv = gamma * invstd * dx)
                slope = case["gamma"] * torch.rsqrt(case["running_var"] + EPS)
                assert not bool(near[:, slope == 0].any()), "a constant channel on the kink"
                step = (4e-3 / slope.masked_fill(slope == 0, 1.0)).view(1, C, 1, 1)
                case["x"] = torch.where(near, case["x"] + step, case["x"]).float().double()
        else:
            raise AssertionError("could not move the pre-activations off the kink")
    if special:
        case["x"][0, 0, 0, 0] = float("nan")
        case["g"][B - 1, min(1, C - 1), H - 1, W - 1] = float("inf")
        case["g"][0, 0, 0, min(1, W - 1)] = float("nan")
    return case


def aten_chain(case, dtype, affine_grads=True):
    """The chain the fused op replaces, in ``dtype`` on the case's device, forward and backward
    -> dict(y, dx[, d_identity][, dgamma, dbeta])"""
    bn = EV.eval_bn(case, dtype)
    # (clones: .to() of a tensor that already has the dtype is the tensor itself, and the case is used again)
    x = case["x"].to(dtype).clone().requires_grad_()
    identity = None if case["identity"] is None else case["identity"].to(dtype).clone().requires_grad_()
    y = bn(x)
    if identity is not None:
        y = y + identity
    if case["mode"]:
        y = F.relu(y)
    y.backward(case["g"].to(dtype))
    out = dict(y=y.detach(), dx=x.grad)
    if identity is not None:
        out["d_identity"] = identity.grad
    if affine_grads:
        out["dgamma"], out["dbeta"] = bn.weight.grad, bn.bias.grad
    return out


def check_frozen_contract(what, fused, aten32, ref64):
    """check_contract; where the fp64 chain is not finite, ATen's bit patterns for the element-wise tensors, and for the
    sums a NaN where ATen has one and ATen's value otherwise (module docstring)"""
    fused, aten32, ref64 = dict(fused), {k: aten32[k] for k in fused}, {k: ref64[k] for k in fused}
    for name in fused:
        odd = ~torch.isfinite(ref64[name]).cpu()
        if not bool(odd.any()):
            continue
        got, want = fused[name].cpu(), aten32[name].cpu()
        if name in ("dgamma", "dbeta"):
            assert torch.equal(torch.isnan(got[odd]), torch.isnan(want[odd])), (what, name, got[odd], want[odd])
            keep = odd & ~torch.isnan(want)
            assert torch.equal(got[keep], want[keep]), (what, name, got[keep], want[keep])
        else:
            odd_np = odd.numpy()
            assert np.array_equal(EV.bits(got)[odd_np], EV.bits(want)[odd_np]), \
                (what, name, "NaN / inf bit patterns differ from ATen's")
        zero = lambda t: t.cpu().masked_fill(odd, 0.0)  # noqa: E731
        fused[name], aten32[name], ref64[name] = zero(fused[name]), zero(aten32[name]), zero(ref64[name])
    check_contract(what, fused, aten32, ref64)


# ---- the whole encoder with frozen statistics, kept off its kinks -----------------------------------------------------
# tests/_encoder_ref.py's ReLU sites with the running statistics in place of the batch's: what condition_encoder and
# preactivation_errors walk when the BatchNorms are frozen.

def _bn_eval(m, t):
    """eval-mode BatchNorm by the module's parameters and running statistics, functionally: no buffer is touched"""
    return F.batch_norm(t, m.running_mean, m.running_var, m.weight, m.bias, False, 0.0, m.eps)


def _eval_block_sites(b, x):
    identity = x if b.downsample is None else _bn_eval(b.downsample[1], b.downsample[0](x))
    v = _bn_eval(b.bn1, b.conv1(x))
    yield b.conv1, v, None
    if hasattr(b, "conv3"):
        v = _bn_eval(b.bn2, b.conv2(F.relu(v)))
        yield b.conv2, v, None
        v = _bn_eval(b.bn3, b.conv3(F.relu(v))) + identity
        yield b.conv3, v, None
    else:
        v = _bn_eval(b.bn2, b.conv2(F.relu(v))) + identity
        yield b.conv2, v, None
    return F.relu(v)


def eval_block_sites(block, x):
    """the sites function of a single frozen BasicBlock or Bottleneck"""
    yield from _eval_block_sites(block, x)


def eval_relu_sites(enc, x):
    """_encoder_ref._relu_sites of a ResnetEncoder whose BatchNorms normalise with their running statistics"""
    e = enc.encoder
    v = _bn_eval(e.bn1, e.conv1(x))
    f0 = F.relu(v)
    yield e.conv1, v, f0
    x = F.max_pool2d(f0, 3, 2, 1)
    for layer in (e.layer1, e.layer2, e.layer3, e.layer4):
        for b in layer:
            x = yield from _eval_block_sites(b, x)


def randomise_bn(net, seed):
    """BatchNorm parameters and running statistics off their initial 1 / 0 (seeded, on the CPU), the counter off 0"""
    import torch.nn as nn
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, nn.BatchNorm2d):
                n = m.num_features
                m.running_mean.copy_(0.1 * torch.randn(n, generator=gen))
                m.running_var.copy_(0.5 + torch.rand(n, generator=gen))
                m.weight.copy_(0.5 + torch.rand(n, generator=gen))
                m.bias.copy_(0.1 * torch.randn(n, generator=gen))
                m.num_batches_tracked.fill_(11)
