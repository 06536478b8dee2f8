"""What the encoder's fused BatchNorm / ReLU / residual ops are tested against, shared by the host-simulator and the GPU
tests: seeded inputs, the ATen chain they replace (run in fp64 as the yardstick and in fp32 beside it) and the contract

    max|fused32 - ref64| <= 2 * max|aten32 - ref64| + 4 u * max|ref64|,   u = 2^-24

per compared tensor (two correct fp32 evaluations that sum in different orders need the factor 2 against each other; the
floor covers tensors ATen happens to hit exactly).

The ReLU is a kink: an entry whose pre-activation lies within rounding of 0 may be cut by one fp32 evaluation and kept by
another, and then a whole upstream gradient appears or vanishes -- no bound on rounding covers that.  So the inputs are
nudged (make_case) until every pre-activation of the fp64 chain is either exactly 0 -- channels with gamma = beta = 0,
where every evaluation yields 0 and drops the gradient, the tie case -- or at least 1e-3 away from 0, four orders of
magnitude above any evaluation's error here."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from _util import report

U = 2.0 ** -24
MODES = {0: "bn", 1: "bn_relu", 2: "bn_add_relu"}
STAGE_SHAPES = [(12, 64, 128, 416), (12, 64, 64, 208), (12, 128, 32, 104), (12, 256, 16, 52), (12, 512, 8, 26)]
ODD_SHAPES = [(1, 3, 2, 2), (2, 5, 3, 3), (3, 2, 5, 263), (1, 4, 7, 131)]
EPS, MOMENTUM = 1e-5, 0.1

# How csrc_enc/scsfm_encoder.hip splits a channel: S = min(ceil(kTargetBlocks / C), ceil(units / kThreads), kMaxSplit)
# workgroups, units = B * H * W / V with V = 4 on the 16-byte path (H * W a multiple of 4), else 1.  The shapes below are
# listed with the S they are meant to hit; splits() recomputes it from the constants in the source, so that a change
# there cannot quietly take a case off its edge.
# ResNet-50's stage outputs (256 ... 2048 channels) at batch 2, sized for the splits S = 8, 4, 2, 1
R50_STAGE_SHAPES = {(2, 256, 32, 128): 8, (2, 512, 32, 64): 4, (2, 1024, 16, 52): 2, (2, 2048, 8, 26): 1}
# the cap; a split that is no power of two and above 32; uneven ranges with the batch boundaries (units 401, 802) inside
# a range on the 16-byte path; uneven ranges on the scalar path
SPLIT_EDGE_SHAPES = {(1, 3, 128, 512): 64, (2, 48, 128, 172): 43, (3, 4, 4, 401): 5, (1, 2, 5, 127): 3}
# those the host simulator runs in under a second a case; S = 43 needs 48 channels of more than 42 * 256 units each, 2 M
# entries, which take it 4 to 8 s a case: that one runs on the GPU only
HOSTSIM_SPLIT_EDGE_SHAPES = [(1, 3, 128, 512), (3, 4, 4, 401), (1, 2, 5, 127)]


def kernel_constants():
    """kTargetBlocks, kMaxSplit, kThreads as csrc_enc/scsfm_encoder.hip defines them"""
    import os
    import re
    src = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "sc-sfmlearner-release_amd",
                       "csrc_enc", "scsfm_encoder.hip")
    with open(src) as f:
        text = f.read()
    return tuple(int(re.search(r"constexpr int %s = (\d+);" % name, text).group(1))
                 for name in ("kTargetBlocks", "kMaxSplit", "kThreads"))


def splits(shape, aligned=True):
    """-> (S, vec) for a contiguous tensor of ``shape``: splits() and the 16-byte condition of the source, in Python"""
    target, most_split, threads = kernel_constants()
    B, C, H, W = shape
    vec = (H * W) % 4 == 0 and aligned
    units = B * (H * W // 4 if vec else H * W)
    return max(1, min(-(-target // C), -(-units // threads), most_split)), vec


def make_case(shape, mode, seed, device="cpu"):
    """x, identity (mode 2), gamma (with negative entries and a zero one), beta, running statistics, the upstream
    gradient; channel 0's mean is 100 x its standard deviation (the cancellation case)."""
    B, C, H, W = shape
    gen = torch.Generator(device=device).manual_seed(seed)
    kw = dict(generator=gen, dtype=torch.float64, device=device)
    x = torch.randn(shape, **kw)
    x = x * (0.5 + torch.rand(1, C, 1, 1, **kw)) + torch.randn(1, C, 1, 1, **kw)
    x[:, 0] = x[:, 0] - x[:, 0].mean()
    x[:, 0] = x[:, 0] / x[:, 0].std().clamp_min(1e-3) * 0.37 + 37.0
    gamma = torch.randn(C, **kw)
    gamma[gamma.abs() < 0.1] = 0.5
    if C > 1:
        gamma[1] = -abs(gamma[1])
    beta = 0.3 * torch.randn(C, **kw)
    zero_ch = C - 1 if C > 2 else None  # gamma = beta = 0: y is exactly 0 there in every evaluation
    if zero_ch is not None:
        gamma[zero_ch], beta[zero_ch] = 0.0, 0.0
    identity = torch.randn(shape, **kw) if mode == 2 else None
    if identity is not None and zero_ch is not None:
        identity[:, zero_ch] = 0.0
    x, gamma, beta = x.float().double(), gamma.float().double(), beta.float().double()  # (fp32-representable)
    if identity is not None:
        identity = identity.float().double()
    if mode:
        for _ in range(4):  # keep the pre-activations off the kink (module docstring)
            v = F.batch_norm(x, None, None, gamma, beta, True, 0.0, EPS)
            if identity is not None:
                v = v + identity
            near = (v.abs() < 1e-3) & (v != 0)
            if zero_ch is not None:
                near[:, zero_ch] = False
            if not bool(near.any()):
                break
            if identity is not None:
                identity = torch.where(near, identity + 0.01, identity).float().double()
            else:
                # (a step that moves the pre-activation by 4e-3 towards +: dv = gamma * invstd * dx)
                invstd = torch.rsqrt(torch.var(x, (0, 2, 3), unbiased=False) + EPS)
                step = (4e-3 / (gamma * invstd).masked_fill(gamma == 0, 1.0)).view(1, C, 1, 1)
                x = torch.where(near, x + step, x).float().double()
        else:
            raise AssertionError("could not move the pre-activations off the kink")
    g = torch.randn(shape, **kw).float().double()
    rm = torch.randn(C, **kw).float().double()
    rv = (0.5 + torch.rand(C, **kw)).float().double()
    return dict(x=x, identity=identity, gamma=gamma, beta=beta, g=g, running_mean=rm, running_var=rv, mode=mode)


def aten_chain(case, dtype, n_forward=1):
    """The chain the fused op replaces -- nn.BatchNorm2d in training mode, the residual add, ReLU -- in ``dtype``:
    n_forward forwards of the same module, then one backward of the last.  -> dict of the compared tensors."""
    x = case["x"].to(dtype).requires_grad_()
    C = x.shape[1]
    bn = nn.BatchNorm2d(C, eps=EPS, momentum=MOMENTUM).to(x.device, dtype).train()
    with torch.no_grad():
        bn.weight.copy_(case["gamma"])
        bn.bias.copy_(case["beta"])
        bn.running_mean.copy_(case["running_mean"])
        bn.running_var.copy_(case["running_var"])
    identity = None if case["identity"] is None else case["identity"].to(dtype).requires_grad_()
    out = {}
    for k in range(n_forward):
        y = bn(x)
        if identity is not None:
            y = y + identity
        if case["mode"]:
            y = F.relu(y)
        if k == 0:
            out["running_mean_1"], out["running_var_1"] = bn.running_mean.clone(), bn.running_var.clone()
    y.backward(case["g"].to(dtype))
    var, mean = torch.var_mean(x.detach(), (0, 2, 3), unbiased=False)
    out.update(y=y.detach(), dx=x.grad, dgamma=bn.weight.grad, dbeta=bn.bias.grad, mean=mean,
               invstd=torch.rsqrt(var + EPS), running_mean=bn.running_mean.clone(), running_var=bn.running_var.clone(),
               num_batches_tracked=int(bn.num_batches_tracked))
    if identity is not None:
        out["d_identity"] = identity.grad
    return out


def check_contract(what, fused, aten32, ref64):
    """the inequality of the module docstring for every tensor of ``fused``; the counter equal as an integer"""
    failures = []
    for name, got in fused.items():
        if name == "num_batches_tracked":
            assert int(got) == ref64[name] == aten32[name], (what, name, int(got), ref64[name])
            continue
        ref = ref64[name].double().cpu()
        assert got.shape == ref.shape, (what, name, got.shape, ref.shape)
        assert bool(torch.isfinite(got).all()), (what, name, "not finite (an output that was not stored?)")
        ef = float((got.double().cpu() - ref).abs().max())
        ea = float((aten32[name].double().cpu() - ref).abs().max())
        bound = 2 * ea + 4 * U * float(ref.abs().max())
        report(f"{what} {name}: max|fused32-ref64| {ef:.3e}  max|aten32-ref64| {ea:.3e}  bound {bound:.3e}")
        if not ef <= bound:
            failures.append((name, ef, ea, bound))
    assert not failures, (what, failures)


def pool_input(shape, seed, device="cpu"):
    """a ReLU output on a coarse grid: exact zeros and ties in most windows"""
    gen = torch.Generator(device=device).manual_seed(seed)
    x = torch.relu(torch.randn(shape, generator=gen, device=device))
    return torch.round(x * 2) / 2


# ---- the whole ResNet-18 encoder kept off its kinks -------------------------------------------------------------------
# A fp32 evaluation of the whole net's gradient jumps by 1e-3 of its scale when one pre-activation within rounding of 0
# is cut by one evaluation and kept by another (measured on ATen's own chain: inputs scaled by 1 + 2^-23 move its
# conv1.weight gradient by 2e-1 of 32, the fp64 chain by 2e-6); two near-equal candidates of a pooling window do the same.
# So the seeded net is conditioned before it is compared: wherever the fp64 chain has a ReLU pre-activation, or a gap
# between the two largest entries of a pooling window, inside (0, KINK_MARGIN), the output channel of the convolution in
# front of it gets new seeded weights, site by site from the stem on, until none is left.  KINK_MARGIN is some 30 times the
# largest fp32 error of a pre-activation here (1e-5), so the comparison measures rounding only.
KINK_MARGIN = 3e-4


def _bn(m, t):
    """training-mode BatchNorm by the module's parameters, functionally: no buffer is touched"""
    return F.batch_norm(t, None, None, m.weight, m.bias, True, 0.0, m.eps)


def _block_sites(b, x):
    """The ReLU sites of one residual block on the input ``x``: a BasicBlock's two (conv1; conv2 with the identity
    added) or a Bottleneck's three (conv1; conv2; conv3 with the identity added).  The down-sample BatchNorm has no ReLU
    behind it (mode 0) and is no site.  Yields as _relu_sites does; the generator's return value is the block's output."""
    identity = x if b.downsample is None else _bn(b.downsample[1], b.downsample[0](x))
    v = _bn(b.bn1, b.conv1(x))
    yield b.conv1, v, None
    if hasattr(b, "conv3"):
        v = _bn(b.bn2, b.conv2(F.relu(v)))
        yield b.conv2, v, None
        v = _bn(b.bn3, b.conv3(F.relu(v))) + identity
        yield b.conv3, v, None
    else:
        v = _bn(b.bn2, b.conv2(F.relu(v))) + identity
        yield b.conv2, v, None
    return F.relu(v)


def block_sites(block, x):
    """the sites function of a single BasicBlock or Bottleneck (for condition_encoder and preactivation_errors)"""
    yield from _block_sites(block, x)


def _relu_sites(enc, x):
    """The ReLU sites of a ResnetEncoder's chain in order (ResNet-18: 17, ResNet-50: 49), evaluated functionally in the
    dtype of ``enc`` and ``x`` (no buffer is touched): yields (the convolution whose output channels feed the site, the
    pre-activation, the ReLU output if a max-pool reads it)."""
    e = enc.encoder
    v = _bn(e.bn1, e.conv1(x))
    f0 = F.relu(v)
    yield e.conv1, v, f0
    x = F.max_pool2d(f0, 3, 2, 1)
    for layer in (e.layer1, e.layer2, e.layer3, e.layer4):
        for b in layer:
            x = yield from _block_sites(b, x)


def _channels_on_a_kink(v, pooled_from, margin):
    bad = ((v.abs() < margin) & (v != 0)).flatten(2).any(2).any(0)
    if pooled_from is not None:
        B, C = pooled_from.shape[:2]
        top = F.unfold(pooled_from, 3, padding=1, stride=2).view(B, C, 9, -1).topk(2, dim=2).values
        gap = top[:, :, 0] - top[:, :, 1]
        bad |= ((gap > 0) & (gap < margin)).any(2).any(0)
    return bad


def condition_encoder(enc64, xs, seed, margin=KINK_MARGIN, max_rounds=20000, sites=_relu_sites):
    """Re-draws convolution output channels of the fp64 ``enc64`` -- a ResnetEncoder(18), or with ``sites=block_sites`` a
    single BasicBlock or Bottleneck -- (fp32-representable values, seeded) until no ReLU pre-activation and no pooling
    gap of its training-mode chain lies in (0, margin) for any input in ``xs``.  -> (rounds used, smallest non-zero
    |pre-activation|, smallest non-zero pooling gap; inf where there is no pooling)."""
    gen = torch.Generator(device=xs[0].device).manual_seed(seed)
    with torch.no_grad():
        for rounds in range(max_rounds):
            lo_v, lo_gap, clean = float("inf"), float("inf"), True
            for group in zip(*[sites(enc64, x) for x in xs]):
                conv = group[0][0]
                bad = torch.zeros(conv.weight.shape[0], dtype=torch.bool, device=conv.weight.device)
                for _, v, pooled_from in group:
                    bad |= _channels_on_a_kink(v, pooled_from, margin)
                if bool(bad.any()):
                    w = conv.weight
                    new = torch.randn(w[bad].shape, generator=gen, device=w.device, dtype=torch.float32) * float(w.std())
                    w[bad] = new.double()
                    clean = False
                    break
                for _, v, pooled_from in group:
                    lo_v = min(lo_v, float(v.abs()[v != 0].min()))
                    if pooled_from is not None:
                        B, C = pooled_from.shape[:2]
                        top = F.unfold(pooled_from, 3, padding=1, stride=2).view(B, C, 9, -1).topk(2, dim=2).values
                        gap = top[:, :, 0] - top[:, :, 1]
                        if bool((gap > 0).any()):
                            lo_gap = min(lo_gap, float(gap[gap > 0].min()))
            if clean:
                return rounds, lo_v, lo_gap
    raise AssertionError("could not move the encoder off its kinks")


def preactivation_errors(m32, m64, xs, sites=_relu_sites):
    """max|v32 - v64| of the pre-activation at every ReLU site, in the sites' order, over the inputs ``xs`` (fp32): the
    ATen chain of ``sites`` evaluated functionally in fp32 through ``m32`` and in fp64 through ``m64``, which holds the
    same values.  A reference quantity: the fused path takes no part in it."""
    with torch.no_grad():
        errs = None
        for x in xs:
            pairs = zip(sites(m32, x), sites(m64, x.double()))
            e = [float((a[1].double() - b[1]).abs().max()) for a, b in pairs]
            errs = e if errs is None else [max(p, q) for p, q in zip(errs, e)]
    return errs


def preactivation_error(m32, m64, xs, sites=_relu_sites):
    """the largest entry of preactivation_errors: what KINK_MARGIN has to stay well above"""
    return max(preactivation_errors(m32, m64, xs, sites))
