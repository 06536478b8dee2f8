"""The depth decoder's fused glue (scsfm_hip.decoder, csrc_nets/scsfm_decoder.hip) against the ATen chain it replaces,
on the GPU: each op at every level shape of configs[1] (batch 12, 256 x 832) and at odd shapes, then the whole fp32
DispResNet, fused against DepthDecoder.forward_reference on the same CUDA tensors.

Forward values are bit-identical.  Backward values are bit-identical except where a reflection-pad corner sums four
padded-gradient entries (ATen adds them with atomics in no fixed order): those entries are bounded by the rounding of
a reordered sum of their terms.  The odd shapes include those around the kernels' 256-element chunk, and each op also
runs a fill of which 40 % are special values (zeros of both signs, infinities, NaN, denormals, saturating and huge
magnitudes: tests/_decoder_ref.py)."""
import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import _decoder_ref as R
from _util import report

pytestmark = pytest.mark.gpu

DEV = "cuda"
U = 2.0 ** -24  # unit roundoff of fp32

# configs[1]: (B, C_a, C_skip, H, W) of up_cat_pad at levels 4..0 (a is conv (i,0)'s output), and (B, C, H, W) of the
# elu_pad inputs b_i and the pad input f4
LEVELS_UP = [(12, 256, 256, 8, 26), (12, 128, 128, 16, 52), (12, 64, 64, 32, 104), (12, 32, 64, 64, 208),
             (12, 16, 0, 128, 416)]
LEVELS_PAD = [(12, 256, 16, 52), (12, 128, 32, 104), (12, 64, 64, 208), (12, 32, 128, 416), (12, 16, 256, 832)]
ODD_UP = R.ODD_UP + R.CHUNK_UP
ODD_PAD = R.ODD_PAD + R.CHUNK_PAD
FLT_MAX = float(np.finfo(np.float32).max)


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


def many_terms(C, H, W, like):
    """True at the entries of an unpadded H x W gradient that the reflection-pad backward sums from more than two padded
    entries (the four (1|H-2, 1|W-2) corners; whole rows / columns when H or W is 3)"""
    x = torch.zeros(1, C, H, W, dtype=torch.float64, device=like.device, requires_grad=True)
    nn.ReflectionPad2d(1)(x).backward(torch.ones(1, C, H + 2, W + 2, dtype=torch.float64, device=like.device))
    return x.grad > 2


def fold_abs(gp):
    """sum of |terms| that the reflection-pad backward adds into each unpadded entry (fp64)"""
    x = torch.zeros(gp.shape[:2] + (gp.shape[2] - 2, gp.shape[3] - 2), dtype=torch.float64, device=gp.device,
                    requires_grad=True)
    nn.ReflectionPad2d(1)(x).backward(gp.double().abs())
    return x.grad


def check_grad(name, got, ref, mask, term_abs):
    """bit-identical outside `mask`; inside it |got - ref| <= 8 u * (sum of |terms| feeding the entry)"""
    assert got.shape == ref.shape
    assert same_bits(got[~mask], ref[~mask]), f"{name}: differs outside the corner entries"
    d = (got[mask].double() - ref[mask].double()).abs()
    bound = 8 * U * term_abs[mask] + 1e-45
    assert bool((d <= bound).all()), f"{name}: corner entries off by {float((d / bound).max()):.2f} x the bound"
    return float((d / bound).max()) if d.numel() else 0.0


def aten_pad_elu(b, elu):
    x = b.clone()  # (a non-leaf, as the conv output the reference's in-place ELU overwrites)
    if elu:
        x = nn.ELU(inplace=True)(x)
    return nn.ReflectionPad2d(1)(x)


def aten_up_cat_pad(a, skip):
    x = F.interpolate(nn.ELU(inplace=True)(a.clone()), scale_factor=2, mode="nearest")
    if skip is not None:
        x = torch.cat([x, skip], 1)
    return nn.ReflectionPad2d(1)(x)


def run_pad(B, C, H, W, elu, seed):
    from scsfm_hip import decoder as D
    g = torch.Generator(device=DEV).manual_seed(seed)
    x0 = torch.randn(B, C, H, W, device=DEV, generator=g)
    gp = torch.randn(B, C, H + 2, W + 2, device=DEV, generator=g)
    x1, x2 = x0.clone().requires_grad_(), x0.clone().requires_grad_()
    out = (D.elu_pad if elu else D.pad)(x1)
    ref = aten_pad_elu(x2, elu)
    assert same_bits(out, ref), "forward"
    out.backward(gp)
    ref.backward(gp)
    return check_grad("g_x", x1.grad, x2.grad, many_terms(C, H, W, x0).expand(x0.shape), fold_abs(gp))


def run_up(B, Ca, Cs, H, W, seed):
    from scsfm_hip import decoder as D
    g = torch.Generator(device=DEV).manual_seed(seed)
    a0 = torch.randn(B, Ca, H, W, device=DEV, generator=g)
    s0 = torch.randn(B, Cs, 2 * H, 2 * W, device=DEV, generator=g) if Cs else None
    gp = torch.randn(B, Ca + Cs, 2 * H + 2, 2 * W + 2, device=DEV, generator=g)
    a1, a2 = a0.clone().requires_grad_(), a0.clone().requires_grad_()
    s1 = s0.clone().requires_grad_() if Cs else None
    s2 = s0.clone().requires_grad_() if Cs else None
    out = D.up_cat_pad(a1, s1)
    ref = aten_up_cat_pad(a2, s2)
    assert out.shape == ref.shape and same_bits(out, ref), "forward"
    out.backward(gp)
    ref.backward(gp)
    terms_a = F.avg_pool2d(fold_abs(gp[:, :Ca]), 2) * 4
    mask_a = F.max_pool2d(many_terms(Ca, 2 * H, 2 * W, a0).double(), 2) > 0
    worst = check_grad("g_a", a1.grad, a2.grad, mask_a.expand(a0.shape), terms_a)
    if Cs:
        worst = max(worst, check_grad("g_skip", s1.grad, s2.grad, many_terms(Cs, 2 * H, 2 * W, s0).expand(s0.shape),
                                      fold_abs(gp[:, Ca:])))
    return worst


@pytest.mark.parametrize("shape", LEVELS_PAD + ODD_PAD + R.R50_PAD)
@pytest.mark.parametrize("elu", [False, True])
def test_pad_matches_aten(shape, elu):
    worst = run_pad(*shape, elu, seed=sum(shape) + elu)
    report(f"decoder pad elu={int(elu)} {shape}: corner entries at {worst:.3f} of their bound")


@pytest.mark.parametrize("shape", LEVELS_UP + ODD_UP + R.R50_UP)
def test_up_cat_pad_matches_aten(shape):
    worst = run_up(*shape, seed=sum(shape))
    report(f"decoder up_cat_pad {shape}: corner entries at {worst:.3f} of their bound")


def same_bits_nan(name, got, ref):
    """the same NaN positions, the same bits elsewhere"""
    assert got.shape == ref.shape, name
    nan = torch.isnan(ref)
    assert torch.equal(torch.isnan(got), nan), f"{name}: NaN positions"
    assert same_bits(got[~nan], ref[~nan]), f"{name}: bits"


def finite_part(gp):
    return torch.where(torch.isfinite(gp), gp, torch.zeros_like(gp))


def check_grad_special(name, got, ref, mask, term_abs, finite_abs):
    """check_grad for gradients that hold special values; term_abs / finite_abs: the sum of |terms| behind each entry,
    over all terms / over the finite ones.  Outside `mask`: the same NaN positions and bits.  Inside it (four or more
    terms, added by ATen in no fixed order): where every term is finite the rounding bound of check_grad; where a term
    is infinite or NaN the same class (NaN, +inf, -inf or finite).  Entries whose finite terms can overflow in one
    order and not in another (their sum of |terms| exceeds FLT_MAX) are left out of both."""
    same_bits_nan(name + " outside the corner entries", got[~mask], ref[~mask])
    g, r, t, no_overflow = got[mask].double(), ref[mask].double(), term_abs[mask], finite_abs[mask] <= FLT_MAX
    tame = torch.isfinite(t) & no_overflow
    d = (g[tame] - r[tame]).abs()
    bound = 8 * U * t[tame] + 1e-45
    assert bool((d <= bound).all()), f"{name}: corner entries off by {float((d / bound).max()):.2f} x the bound"
    wild = ~torch.isfinite(t) & no_overflow
    for cls in (torch.isnan, torch.isposinf, torch.isneginf):
        assert torch.equal(cls(g[wild]), cls(r[wild])), f"{name}: {cls.__name__} at the corner entries"
    return int(tame.sum()), int(wild.sum())


def _special(shape, rng):
    return torch.from_numpy(R.fill(shape, "special", rng)).to(DEV)


@pytest.mark.parametrize("shape", [(2, 5, 3, 3), (1, 1, 2, 257), (3, 2, 5, 263), (2, 8, 16, 52)])
@pytest.mark.parametrize("elu", [False, True])
def test_pad_matches_aten_on_special_values(shape, elu):
    """Measured on an MI355X: ATen and the kernels agree bit for bit on every entry outside the corners, denormal
    g * (r + 1) and expm1f at each of R.SPECIALS included (neither side flushes denormals), here and for up_cat_pad."""
    from scsfm_hip import decoder as D
    B, C, H, W = shape
    rng = np.random.default_rng(sum(shape) + elu)
    x0, gp = _special(shape, rng), _special((B, C, H + 2, W + 2), rng)
    x1, x2 = x0.clone().requires_grad_(), x0.clone().requires_grad_()
    out = (D.elu_pad if elu else D.pad)(x1)
    ref = aten_pad_elu(x2, elu)
    same_bits_nan("forward", out, ref)
    out.backward(gp)
    ref.backward(gp)
    n = check_grad_special("g_x", x1.grad, x2.grad, many_terms(C, H, W, x0).expand(x0.shape), fold_abs(gp),
                           fold_abs(finite_part(gp)))
    report(f"decoder pad elu={int(elu)} {shape} special values: as ATen ({n[0]} bounded, {n[1]} classed corner entries)")


@pytest.mark.parametrize("shape", [(1, 3, 2, 1, 1), (2, 7, 3, 3, 5), (1, 2, 0, 2, 129), (1, 4, 4, 5, 131),
                                   (2, 16, 8, 16, 52)])
def test_up_cat_pad_matches_aten_on_special_values(shape):
    from scsfm_hip import decoder as D
    B, Ca, Cs, H, W = shape
    rng = np.random.default_rng(sum(shape))
    a0 = _special((B, Ca, H, W), rng)
    s0 = _special((B, Cs, 2 * H, 2 * W), rng) if Cs else None
    gp = _special((B, Ca + Cs, 2 * H + 2, 2 * W + 2), rng)
    a1, a2 = a0.clone().requires_grad_(), a0.clone().requires_grad_()
    s1 = s0.clone().requires_grad_() if Cs else None
    s2 = s0.clone().requires_grad_() if Cs else None
    out = D.up_cat_pad(a1, s1)
    ref = aten_up_cat_pad(a2, s2)
    same_bits_nan("forward", out, ref)
    out.backward(gp)
    ref.backward(gp)
    terms_a = F.avg_pool2d(fold_abs(gp[:, :Ca]), 2) * 4
    mask_a = F.max_pool2d(many_terms(Ca, 2 * H, 2 * W, a0).double(), 2) > 0
    n = check_grad_special("g_a", a1.grad, a2.grad, mask_a.expand(a0.shape), terms_a,
                           F.avg_pool2d(fold_abs(finite_part(gp[:, :Ca])), 2) * 4)
    if Cs:
        check_grad_special("g_skip", s1.grad, s2.grad, many_terms(Cs, 2 * H, 2 * W, s0).expand(s0.shape),
                           fold_abs(gp[:, Ca:]), fold_abs(finite_part(gp[:, Ca:])))
    report(f"decoder up_cat_pad {shape} special values: as ATen ({n[0]} bounded, {n[1]} classed corner entries of g_a)")


def test_upsample_backward_sums_children_row_major_from_zero():
    """ATen's upsample_nearest2d backward sums the 2 x 2 children from 0 in row-major order: with children
    (1, u / -1, u), u = 2^-24, that gives ((1 + u) - 1) + u = u, column-major would give 2u."""
    from scsfm_hip import decoder as D
    u = 2.0 ** -24
    gp = torch.zeros(1, 1, 8, 8, device=DEV)  # a 3 x 3 -> 6 x 6 upsampled: a[1][1]'s children are no border entries
    gp[0, 0, 3:5, 3:5] = torch.tensor([[1.0, u], [-1.0, u]], device=DEV)
    a1 = torch.ones(1, 1, 3, 3, device=DEV, requires_grad=True)  # (ELU' = 1 at a > 0)
    a2 = torch.ones(1, 1, 3, 3, device=DEV, requires_grad=True)
    D.up_cat_pad(a1).backward(gp)
    aten_up_cat_pad(a2, None).backward(gp)
    assert float(a2.grad[0, 0, 1, 1]) == u, "ATen's order is not row-major from zero"
    assert same_bits(a1.grad, a2.grad)


def _nets(seed=0):
    import models
    torch.manual_seed(seed)
    return models.DispResNet(18, False).to(DEV)


def _outputs(net, x, fused):
    feats = net.encoder(x)
    dec = net.decoder
    assert dec.fused_path_applies(feats)
    return dec.forward_fused(feats) if fused else dec.forward_reference(feats)


@pytest.fixture
def deterministic_miopen():
    """MIOpen's solvers for some of these shapes (B = 2) are not reproducible from call to call (the 512-channel
    convolution of block 0 differs by ~1e-6 between two calls on the same input); ask for deterministic ones."""
    old = torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = True, False
    yield
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = old


@pytest.mark.parametrize("mode", ["train", "eval", "no_grad"])
def test_disp_resnet_outputs_match_the_reference(mode, deterministic_miopen):
    """Fused against reference on the same encoder features: bit-identical whenever the reference reproduces itself
    (the glue adds no difference of its own); in any case no further apart than two reference runs."""
    net = _nets()
    net.train(mode == "train")
    x = torch.randn(2, 3, 128, 416, device=DEV, generator=torch.Generator(device=DEV).manual_seed(3))
    with torch.set_grad_enabled(mode != "no_grad"):
        feats = net.encoder(x)
        ref1 = net.decoder.forward_reference(feats)
        got = net.decoder.forward_fused(feats)
        ref2 = net.decoder.forward_reference(feats)
        top = net(x)
    assert len(got) == 4 and (len(top) == 4 if mode == "train" else top.shape == got[0].shape)
    reproducible = all(same_bits(a, b) for a, b in zip(ref1, ref2))
    for s, (a, b, c) in enumerate(zip(got, ref1, ref2)):
        if reproducible:
            assert same_bits(a, b), f"scale {s}"
        else:
            assert float((a - b).abs().max()) <= 3 * float((c - b).abs().max()), f"scale {s}"
    report(f"DispResNet outputs {mode}: reference reproducible {reproducible}, fused bit-identical "
           f"{all(same_bits(a, b) for a, b in zip(got, ref1))}")


@pytest.mark.parametrize("num_scales", [1, 4])
def test_disp_resnet_gradients_within_the_reference_spread(num_scales, deterministic_miopen):
    """Parameter gradients (encoder and decoder) of a loss over the first num_scales outputs: fused against the
    reference, next to two reference runs against each other (MIOpen's weight-gradient reductions are not ordered).
    num_scales = 4 also exercises the shared Q_i, whose border sums autograd reassociates."""
    net = _nets(1).train()
    x = torch.randn(2, 3, 128, 416, device=DEV, generator=torch.Generator(device=DEV).manual_seed(5))
    w = [torch.randn(2, 1, 128 // 2 ** s, 416 // 2 ** s, device=DEV,
                     generator=torch.Generator(device=DEV).manual_seed(10 + s)) for s in range(4)]

    def grads(fused):
        net.zero_grad(set_to_none=True)
        outs = _outputs(net, x, fused)
        sum((o * w[s]).sum() for s, o in enumerate(outs[:num_scales])).backward()
        return [p.grad.clone() for p in net.parameters() if p.grad is not None]

    ref1, ref2, got = grads(False), grads(False), grads(True)
    assert len(got) == len(ref1)
    worst_rel, worst_spread = 0.0, 0.0
    for g, r1, r2 in zip(got, ref1, ref2):
        scale = float(r1.abs().max()) + 1e-30
        d = float((g - r1).abs().max())
        spread = float((r2 - r1).abs().max())
        worst_rel = max(worst_rel, d / scale)
        worst_spread = max(worst_spread, spread / scale)
        assert d <= 3 * spread + 1e-5 * scale, (tuple(g.shape), d, spread, scale)
    report(f"DispResNet gradients num_scales={num_scales}: fused vs reference worst {worst_rel:.2e} of scale, "
           f"reference vs reference {worst_spread:.2e}")


# ---- the decoder under ResNet-50's encoder: skips of 256, 512 and 1024 channels, f4 of 2048 ----------------------------
@pytest.fixture(scope="module")
def resnet50_decoder():
    """DispResNet(50)'s decoder in training mode and the encoder's five features of a 2 x 3 x 64 x 128 image, detached:
    the comparison starts behind the encoder (whose fp32 error at this depth is
    test_gpu_encoder_fused.test_resnet50_encoder_takes_the_fused_path's subject)"""
    import models
    torch.manual_seed(2)
    net = models.DispResNet(50, False).to(DEV).train()
    x = torch.randn(2, 3, 64, 128, device=DEV, generator=torch.Generator(device=DEV).manual_seed(3))
    with torch.no_grad():
        feats = [f.clone() for f in net.encoder(x)]
    assert [tuple(f.shape) for f in feats] == [(2, 64, 32, 64), (2, 256, 16, 32), (2, 512, 8, 16), (2, 1024, 4, 8),
                                               (2, 2048, 2, 4)]
    return net.decoder, feats


PATHS = ["forward_fused", "forward_fused_bias"]


@pytest.mark.parametrize("path", PATHS)
def test_resnet50_decoder_outputs_match_the_reference(path, resnet50_decoder, deterministic_miopen):
    """as test_disp_resnet_outputs_match_the_reference, for both fused paths; forward() takes the folded-bias one"""
    dec, feats = resnet50_decoder
    assert dec.fused_path_applies(feats) and dec.bias_path_applies()
    ref1 = dec.forward_reference(feats)
    got = getattr(dec, path)(feats)
    ref2 = dec.forward_reference(feats)
    top = dec(feats)
    assert len(got) == len(top) == len(ref1) == 4
    assert [tuple(o.shape) for o in got] == [(2, 1, 64 >> s, 128 >> s) for s in range(4)]
    reproducible = all(same_bits(a, b) for a, b in zip(ref1, ref2))
    for s, (a, b, c, t) in enumerate(zip(got, ref1, ref2, top)):
        if reproducible:
            assert same_bits(a, b) and same_bits(t, b), f"scale {s}"
        else:
            assert float((a - b).abs().max()) <= 3 * float((c - b).abs().max()), f"scale {s}"
    report(f"DepthDecoder under ResNet-50 {path}: reference reproducible {reproducible}, fused bit-identical "
           f"{all(same_bits(a, b) for a, b in zip(got, ref1))}")


@pytest.mark.parametrize("num_scales", [1, 4])
@pytest.mark.parametrize("path", PATHS)
def test_resnet50_decoder_gradients_within_the_reference_spread(path, num_scales, resnet50_decoder,
                                                                deterministic_miopen):
    """Gradients of a loss over the first num_scales outputs with respect to the decoder's parameters and the five
    features: fused against the reference, next to two reference runs against each other."""
    dec, feats = resnet50_decoder
    w = [torch.randn(2, 1, 64 >> s, 128 >> s, device=DEV, generator=torch.Generator(device=DEV).manual_seed(10 + s))
         for s in range(4)]

    def grads(forward):
        dec.zero_grad(set_to_none=True)
        leaves = [f.clone().requires_grad_() for f in feats]
        outs = forward(leaves)
        sum((o * w[s]).sum() for s, o in enumerate(outs[:num_scales])).backward()
        out = {f"feature {i}": f.grad for i, f in enumerate(leaves)}
        out.update({n: p.grad.clone() for n, p in dec.named_parameters() if p.grad is not None})
        return out

    ref1, ref2, got = grads(dec.forward_reference), grads(dec.forward_reference), grads(getattr(dec, path))
    assert list(got) == list(ref1) and len(got) == 5 + 2 * (10 + num_scales)
    worst_rel, worst_spread = 0.0, 0.0
    for n in got:
        g, r1, r2 = got[n], ref1[n], ref2[n]
        assert g is not None and g.shape == r1.shape, n
        scale = float(r1.abs().max()) + 1e-30
        d = float((g - r1).abs().max())
        spread = float((r2 - r1).abs().max())
        worst_rel = max(worst_rel, d / scale)
        worst_spread = max(worst_spread, spread / scale)
        assert d <= 3 * spread + 1e-5 * scale, (n, tuple(g.shape), d, spread, scale)
    report(f"DepthDecoder under ResNet-50 {path} num_scales={num_scales}: fused vs reference worst {worst_rel:.2e} of "
           f"scale, reference vs reference {worst_spread:.2e}")


def test_resnet50_decoder_routes_the_layers_resnet18s_does(resnet50_decoder, monkeypatch):
    """The decoder's own channel counts do not depend on the encoder, so scsfm_hip.conv_wrw and scsfm_hip.decoder_dgrad
    take the same convolutions (by their index in DepthDecoder.decoder) under ResNet-50's features as under
    ResNet-18's, on both fused paths."""
    import models
    from scsfm_hip import conv_wrw as CW, decoder_dgrad as DG
    dec50, feats50 = resnet50_decoder
    torch.manual_seed(2)
    dec18 = models.DispResNet(18, False).decoder.to(DEV).train()
    feats18 = [torch.randn(f.shape[0], c, *f.shape[2:], device=DEV) for f, c in zip(feats50, dec18.num_ch_enc)]
    seen = []
    real_wrw, real_tail = CW.applies, DG.applies

    def wrw_applies(x, m):
        seen.append(("wrw", id(m), real_wrw(x, m)))
        return seen[-1][2]

    def tail_applies(b, bias, head):
        seen.append(("tail", id(head), real_tail(b, bias, head)))
        return seen[-1][2]

    monkeypatch.setattr(CW, "applies", wrw_applies)
    monkeypatch.setattr(DG, "applies", tail_applies)

    def routes(dec, feats, path):
        index = {id(dec._conv(k)): k for k in range(len(dec.decoder))}
        del seen[:]
        with torch.no_grad():
            getattr(dec, path)(feats)
        return [(kind, index[m], took) for kind, m, took in seen]

    for path in PATHS:
        r18, r50 = routes(dec18, feats18, path), routes(dec50, feats50, path)
        assert r18 == r50, path
        taken = sorted(k for kind, k, took in r50 if kind == "wrw" and took)
        assert taken == [k for k in sorted(k for kind, k, _ in r50 if kind == "wrw") if k in (6, 7, 8, 9, 10, 11, 12)], path
        assert len(taken) >= 6 and (path == "forward_fused" or ("tail", 10, True) in r50)
