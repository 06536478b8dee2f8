"""What the fused stem (relu(bn(x)) + max-pool, include/scsfm_stem.h) is tested against, shared by the host-simulator
and the GPU tests: the shapes, seeded inputs kept off both kinks of the chain, the ATen chain in a given dtype, and the
bound on dx against the unfused pair of ops.

The shapes are the smallest at which each mechanism of the kernels can break: windows that are all clipped, H = 1, odd
H and W (scalar kernels), rows wider than a wave, the 16-byte kernels at even sizes, with an odd H and several bands per
plane, and a row wider than one workgroup's 1024 columns (the segment path)."""
import torch
import torch.nn as nn
import torch.nn.functional as F

import _encoder_ref as R

SMALL_SHAPES = [(1, 3, 2, 2), (1, 2, 1, 2), (2, 5, 3, 3), (3, 2, 5, 263), (1, 4, 7, 131), (2, 4, 8, 16),
                (2, 3, 33, 516), (1, 2, 3, 1028)]
STEM_SHAPE = (12, 64, 128, 416)
U = R.U


def pooled_shape(shape):
    B, C, H, W = shape
    return B, C, (H - 1) // 2 + 1, (W - 1) // 2 + 1


def make_case(shape, seed, device="cpu"):
    """_encoder_ref.make_case(shape, 1, seed) plus a seeded gradient for the pooled map"""
    case = R.make_case(shape, 1, seed, device=device)
    gen = torch.Generator(device=device).manual_seed(seed + 12345)
    case["g_pool"] = torch.randn(pooled_shape(shape), generator=gen, dtype=torch.float64, device=device).float().double()
    return case


def _pre_activation(case):
    return F.batch_norm(case["x"], None, None, case["gamma"], case["beta"], True, 0.0, R.EPS)


def off_the_kinks(case, margin=R.KINK_MARGIN):
    """(no ReLU pre-activation of the fp64 chain in (0, 1e-3) in magnitude, no gap between a pooling window's two
    largest entries in (0, margin)) -> bool"""
    v = _pre_activation(case)
    if bool(((v.abs() < 1e-3) & (v != 0)).any()):
        return False
    f0 = F.relu(v)
    B, C = f0.shape[:2]
    top = F.unfold(f0, 3, padding=1, stride=2).view(B, C, 9, -1).topk(2, dim=2).values
    gap = top[:, :, 0] - top[:, :, 1]
    return not bool(((gap > 0) & (gap < margin)).any())


def make_conditioned_case(shape, seed, device="cpu", margin=R.KINK_MARGIN, max_rounds=40):
    """make_case with x nudged until the fp64 chain is off both kinks: every ReLU pre-activation exactly 0 or at least
    1e-3 from it (make_case's rule), and the two largest entries of every pooling window equal (ties of ReLU zeros) or at
    least ``margin`` apart.  A window's winner is raised by 4e-3 (in the pre-activation) where the gap is too small;
    raises if that does not settle."""
    case = make_case(shape, seed, device=device)
    C = shape[1]
    for _ in range(max_rounds):
        if off_the_kinks(case, margin):
            return case
        x, gamma = case["x"], case["gamma"]
        invstd = torch.rsqrt(torch.var(x, (0, 2, 3), unbiased=False) + R.EPS)
        step = (4e-3 / (gamma * invstd).masked_fill(gamma == 0, 1.0)).view(1, C, 1, 1)
        v = _pre_activation(case)
        near = (v.abs() < 1e-3) & (v != 0)
        if not bool(near.any()):
            f0 = F.relu(v)
            B = f0.shape[0]
            _, idx = F.max_pool2d(f0, 3, 2, 1, return_indices=True)
            top = F.unfold(f0, 3, padding=1, stride=2).view(B, C, 9, -1).topk(2, dim=2).values
            gap = (top[:, :, 0] - top[:, :, 1]).view(idx.shape)
            bad = (gap > 0) & (gap < margin)
            near = _winners(idx, bad, f0.shape)  # (a winner of several such windows is raised once)
        case["x"] = torch.where(near, x + step, x).float().double()
    raise AssertionError(f"could not move {shape} seed {seed} off its kinks")


def _winners(idx, bad, shape):
    """mask[B,C,H,W] of the entries that win a window flagged in ``bad``"""
    B, C, H, W = shape
    plane = torch.arange(B * C, device=idx.device).view(B, C, 1, 1) * (H * W)
    flat = (idx + plane)[bad]
    mask = torch.zeros(B * C * H * W, dtype=torch.bool, device=idx.device)
    mask[flat] = True
    return mask.view(shape)


def aten_chain(case, dtype, n_forward=1, with_f0_grad=True):
    """nn.BatchNorm2d in training mode, ReLU, F.max_pool2d(3, 2, 1) in ``dtype``: n_forward forwards of the same module,
    then one backward of the last with case["g_pool"] on the pooled map and (with_f0_grad) case["g"] on f0."""
    x = case["x"].to(dtype).requires_grad_()
    C = x.shape[1]
    bn = nn.BatchNorm2d(C, eps=R.EPS, momentum=R.MOMENTUM).to(x.device, dtype).train()
    with torch.no_grad():
        bn.weight.copy_(case["gamma"])
        bn.bias.copy_(case["beta"])
        bn.running_mean.copy_(case["running_mean"])
        bn.running_var.copy_(case["running_var"])
    out = {}
    for k in range(n_forward):
        f0 = F.relu(bn(x))
        pooled = F.max_pool2d(f0, 3, 2, 1)
        if k == 0:
            out["running_mean_1"], out["running_var_1"] = bn.running_mean.clone(), bn.running_var.clone()
    loss = (pooled * case["g_pool"].to(dtype)).sum()
    if with_f0_grad:
        loss = loss + (f0 * case["g"].to(dtype)).sum()
    loss.backward()
    var, mean = torch.var_mean(x.detach(), (0, 2, 3), unbiased=False)
    out.update(f0=f0.detach(), pooled=pooled.detach(), dx=x.grad, dgamma=bn.weight.grad, dbeta=bn.bias.grad, mean=mean,
               invstd=torch.rsqrt(var + R.EPS), running_mean=bn.running_mean.clone(),
               running_var=bn.running_var.clone(), num_batches_tracked=int(bn.num_batches_tracked))
    return out


def ulps_apart(a, b):
    """largest distance of two fp32 tensors in units of the last place of the larger magnitude (0 where both are 0)"""
    a, b = a.double().cpu(), b.double().cpu()
    scale = torch.maximum(a.abs(), b.abs())
    ulp = torch.where(scale > 0, 2.0 ** (torch.floor(torch.log2(scale.clamp_min(1e-300))) - 23), torch.ones_like(scale))
    return float(((a - b).abs() / ulp).max())


def dx_bound(gprime, xhat, gamma, invstd, dgamma, dbeta):
    """Per channel, 8 u |gamma invstd| (max|g'| + |dbeta| / N + max|xhat| |dgamma| / N): what one-ulp differences of the
    two per-channel sums, and the roundings of the expression itself, can move dx = gamma invstd (g' - dbeta / N - xhat
    dgamma / N) by.  All arguments are the unfused pair's own tensors (fp32), N entries per channel."""
    B, C, H, W = gprime.shape
    N = B * H * W
    d = lambda t: t.double().cpu()  # noqa: E731
    mg = d(gprime.abs().amax((0, 2, 3)))
    mx = d(xhat.abs().amax((0, 2, 3)))
    return 8 * U * (d(gamma) * d(invstd)).abs() * (mg + d(dbeta).abs() / N + mx * d(dgamma).abs() / N)


def check_backward_against_pair(what, stem, pair, case_tensors):
    """stem / pair: dicts with dx, dgamma, dbeta (fp32); case_tensors: gprime, xhat, gamma, invstd of the pair.  dgamma and
    dbeta within one ulp, dx within dx_bound per channel."""
    from _util import report
    for name in ("dbeta", "dgamma"):
        d = ulps_apart(stem[name], pair[name])
        report(f"{what} {name}: {d:.2f} ulp from the unfused pair's")
        assert d <= 1.0, (what, name, d)
    bound = dx_bound(case_tensors["gprime"], case_tensors["xhat"], case_tensors["gamma"], case_tensors["invstd"],
                     pair["dgamma"], pair["dbeta"])
    err = (stem["dx"].double() - pair["dx"].double()).abs().amax((0, 2, 3)).cpu()
    worst = float((err / bound.clamp_min(1e-300)).max()) if bool((bound > 0).any()) else 0.0
    report(f"{what} dx: max |stem - pair| {float(err.max()):.3e}, worst channel at {worst:.3f} of its bound")
    assert bool((err <= bound).all()), (what, err.tolist(), bound.tolist())
