"""The decoder's glue with folded biases (scsfm_hip.decoder_bias, csrc_decb/scsfm_decoder_bias.hip) on the GPU, against
the ATen chain it replaces, at the shapes of tests/test_decbias_hostsim.py: the forward bit-identical to
conv-output + bias -> ELU / upsample / cat / pad (or sigmoid -> mul -> add), the activation gradients bit-identical to
scsfm_hip.decoder's on the biased input, the bias gradient within 2^-23 * sum|terms| of the chain's sum done in fp64 (ATen's fp32
sum is printed beside it).  Then the whole fp32 DispResNet: forward_fused_bias against forward_fused and
forward_reference, and a captured graph of forward plus backward against the eager run."""
import itertools

import pytest
import torch
import torch.nn.functional as F

import _decoder_ref as R
from _util import report

pytestmark = pytest.mark.gpu

DEV = "cuda"
ELU_SHAPES = [(B, C, H, W) for B, C, H in itertools.product((1, 2), (1, 3, 5), (2, 3, 5))
              for W in (2, 3, 254, 255, 256, 257, 258, 513)] + R.R50_PAD + [(2, 256, 4, 8)]  # (... and channel-sized)
UP_SHAPES = [(B, Ca, Cs, H, W) for B, (Ca, Cs), H in itertools.product((1, 2), ((1, 0), (3, 2), (5, 0)), (1, 2, 3))
             for W in (2, 3, 127, 128, 129)] + R.R50_UP  # (... and the levels under ResNet-50's skips)
HEAD_SHAPES = [(B, 1, H, W) for B in (1, 2) for H, W in ((2, 2), (5, 51), (1, 255), (16, 16), (1, 257))] + \
    [(2, 3, 1, 257), (2, 1, 64, 208)]


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def _rand(gen, *shape):
    return torch.randn(*shape, device=DEV, generator=gen)


def _col(bias):
    return bias.view(1, -1, 1, 1)


def _bias_check(name, got, stored, aten32, worst):
    """|got - sum64| <= 2^-23 * sum|terms| per channel, where the terms are the activation gradient the backward stored
    (bit for bit ATen's but for the pad corners) and sum64 is the chain's last step, grad_output.sum((0, 2, 3)), done
    in fp64 on it: the bound of tests/test_decbias_hostsim.py, which a fixed-order fp64 sum rounded once to fp32 meets
    with a factor of four to spare.  (Against a chain that is fp64 from its inputs on, the fp32 roundings of the terms
    themselves would be measured, which the bias sum does not make and ATen's has as well.)  -> the worst ratios of
    error to bound so far (ours, ATen's fp32 sum)"""
    g64, mag = stored.double().sum((0, 2, 3)), stored.double().abs().sum((0, 2, 3))
    bound = 2.0 ** -23 * mag
    d, d_aten = (got.double() - g64).abs(), (aten32.double() - g64).abs()
    assert bool((d <= bound).all()), (name, d.tolist(), bound.tolist())
    return max(worst[0], float((d / bound).max())), max(worst[1], float((d_aten / bound).max()))


def test_bias_elu_pad_against_the_aten_chain():
    from scsfm_hip import decoder as D, decoder_bias as DB
    gen = torch.Generator(device=DEV).manual_seed(1)
    worst = (0.0, 0.0)
    for shape in ELU_SHAPES:
        B, C, H, W = shape
        x, bias, gp = _rand(gen, *shape), _rand(gen, C), _rand(gen, B, C, H + 2, W + 2)
        x1, b1 = x.clone().requires_grad_(), bias.clone().requires_grad_()
        out = DB.elu_pad(x1, b1)
        out.backward(gp)
        x2, b2 = x.clone().requires_grad_(), bias.clone().requires_grad_()
        ref = F.pad(F.elu(x2 + _col(b2)), (1, 1, 1, 1), mode="reflect")
        assert same_bits(out, ref), shape
        ref.backward(gp)
        x3 = (x + _col(bias)).requires_grad_()
        D.elu_pad(x3).backward(gp)
        assert same_bits(x1.grad, x3.grad), shape
        worst = _bias_check(f"elu_pad {shape}", b1.grad, x1.grad, b2.grad, worst)
        # a second call gives the same bits; a frozen bias gets no gradient
        x5, b5 = x.clone().requires_grad_(), bias.clone().requires_grad_()
        DB.elu_pad(x5, b5).backward(gp)
        assert same_bits(b5.grad, b1.grad) and same_bits(x5.grad, x1.grad), shape
        x6 = x.clone().requires_grad_()
        DB.elu_pad(x6, bias).backward(gp)
        assert same_bits(x6.grad, x1.grad), shape
    report(f"bias_elu_pad: bias gradient at most {worst[0]:.3f} of 2^-23 sum|terms| from the fp64 sum "
           f"(ATen's fp32 sum: {worst[1]:.3f}) over {len(ELU_SHAPES)} shapes")


def test_bias_up_cat_pad_against_the_aten_chain():
    from scsfm_hip import decoder as D, decoder_bias as DB
    gen = torch.Generator(device=DEV).manual_seed(2)
    worst = (0.0, 0.0)

    def chain(a, b, skip):
        up = F.interpolate(F.elu(a + _col(b)), scale_factor=2, mode="nearest")
        return F.pad(up if skip is None else torch.cat([up, skip], 1), (1, 1, 1, 1), mode="reflect")

    for shape in UP_SHAPES:
        B, Ca, Cs, H, W = shape
        a, bias = _rand(gen, B, Ca, H, W), _rand(gen, Ca)
        skip = _rand(gen, B, Cs, 2 * H, 2 * W) if Cs else None
        gp = _rand(gen, B, Ca + Cs, 2 * H + 2, 2 * W + 2)
        leaf = lambda t: None if t is None else t.clone().requires_grad_()  # noqa: E731
        a1, b1, s1 = leaf(a), leaf(bias), leaf(skip)
        out = DB.up_cat_pad(a1, b1, s1)
        out.backward(gp)
        a2, b2, s2 = leaf(a), leaf(bias), leaf(skip)
        ref = chain(a2, b2, s2)
        assert same_bits(out, ref), shape
        ref.backward(gp)
        a3, s3 = (a + _col(bias)).requires_grad_(), leaf(skip)
        D.up_cat_pad(a3, s3).backward(gp)
        assert same_bits(a1.grad, a3.grad) and (skip is None or same_bits(s1.grad, s3.grad)), shape
        worst = _bias_check(f"up_cat_pad {shape}", b1.grad, a1.grad, b2.grad, worst)
        a5, b5, s5 = leaf(a), leaf(bias), leaf(skip)
        DB.up_cat_pad(a5, b5, s5).backward(gp)
        assert same_bits(b5.grad, b1.grad) and same_bits(a5.grad, a1.grad), shape
    report(f"bias_up_cat_pad: bias gradient at most {worst[0]:.3f} of 2^-23 sum|terms| from the fp64 sum "
           f"(ATen's fp32 sum: {worst[1]:.3f}) over {len(UP_SHAPES)} shapes")


def test_disp_head_against_the_aten_chain():
    """Forward and activation gradient bit-identical to ATen's conv + bias -> sigmoid -> mul -> add (alpha an int, beta a
    float, as DepthDecoder holds them)."""
    from scsfm_hip import decoder_bias as DB
    gen = torch.Generator(device=DEV).manual_seed(3)
    worst = (0.0, 0.0)
    alpha, beta = 10, 0.01
    for shape in HEAD_SHAPES:
        B, C, H, W = shape
        x, bias, g = 3 * _rand(gen, *shape), _rand(gen, C), _rand(gen, *shape)
        x1, b1 = x.clone().requires_grad_(), bias.clone().requires_grad_()
        out = DB.disp_head(x1, b1, alpha, beta)
        out.backward(g)
        x2, b2 = x.clone().requires_grad_(), bias.clone().requires_grad_()
        ref = alpha * torch.sigmoid(x2 + _col(b2)) + beta
        ref.backward(g)
        ulp = int((bits(out).long() - bits(ref).long()).abs().max())
        assert same_bits(out, ref), (shape, f"{ulp} ulp")
        assert same_bits(x1.grad, x2.grad), shape
        worst = _bias_check(f"disp_head {shape}", b1.grad, x1.grad, b2.grad, worst)
        x5, b5 = x.clone().requires_grad_(), bias.clone().requires_grad_()
        DB.disp_head(x5, b5, alpha, beta).backward(g)
        assert same_bits(b5.grad, b1.grad) and same_bits(x5.grad, x1.grad), shape
    report(f"disp_head: forward and activation gradient bit-identical to ATen; bias gradient at most {worst[0]:.3f} of "
           f"2^-23 sum|terms| from the fp64 sum (ATen's fp32 sum: {worst[1]:.3f}) over {len(HEAD_SHAPES)} shapes")


def test_rejections_and_frozen_biases():
    from scsfm_hip import decoder_bias as DB
    x = torch.randn(1, 3, 4, 5, device=DEV)
    with pytest.raises(ValueError):
        DB.elu_pad(x, torch.zeros(4, device=DEV))
    with pytest.raises(ValueError):
        DB.elu_pad(x, torch.zeros(3))
    with pytest.raises(ValueError):
        DB.disp_head(x.double(), torch.zeros(3, device=DEV), 10, 0.01)
    with pytest.raises(ValueError):
        DB.up_cat_pad(x, torch.zeros(3, device=DEV), torch.zeros(1, 2, 8, 11, device=DEV))


def _nets(seed=0):
    import models
    torch.manual_seed(seed)
    return models.DispResNet(18, False).to(DEV)


@pytest.fixture
def deterministic_miopen():
    """as tests/test_gpu_decoder_fused.py: MIOpen's default solvers for some of these shapes are not reproducible"""
    old = torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = True, False
    yield
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = old


@pytest.mark.parametrize("mode", ["train", "no_grad"])
def test_disp_resnet_outputs_match_forward_fused(mode, deterministic_miopen):
    """forward_fused_bias against forward_fused on the same features: bit-identical whenever forward_fused reproduces
    itself, otherwise no further apart than 3 x two runs of it.  forward() takes the new path."""
    from models.DispResNet import DepthDecoder
    net = _nets()
    net.train(mode == "train")
    x = torch.randn(2, 3, 128, 416, device=DEV, generator=torch.Generator(device=DEV).manual_seed(3))
    with torch.set_grad_enabled(mode != "no_grad"):
        feats = net.encoder(x)
        assert net.decoder.fused_path_applies(feats) and net.decoder.bias_path_applies()
        old1 = net.decoder.forward_fused(feats)
        got = net.decoder.forward_fused_bias(feats)
        old2 = net.decoder.forward_fused(feats)
        calls = []
        orig = DepthDecoder.forward_fused_bias
        DepthDecoder.forward_fused_bias = lambda self, f: calls.append(1) or orig(self, f)
        try:
            top = net.decoder(feats)
        finally:
            DepthDecoder.forward_fused_bias = orig
    assert calls == [1] and len(got) == len(top) == 4
    reproducible = all(same_bits(a, b) for a, b in zip(old1, old2))
    for s, (a, b, c, t) in enumerate(zip(got, old1, old2, top)):
        if reproducible:
            assert same_bits(a, b) and same_bits(t, b), f"scale {s}"
        else:
            assert float((a - b).abs().max()) <= 3 * float((c - b).abs().max()), f"scale {s}"
    report(f"DispResNet outputs {mode}: forward_fused reproducible {reproducible}, forward_fused_bias bit-identical "
           f"{all(same_bits(a, b) for a, b in zip(got, old1))}")


@pytest.mark.parametrize("num_scales", [1, 4])
def test_disp_resnet_gradients_within_the_reference_spread(num_scales, deterministic_miopen):
    """Parameter gradients of a loss over the first num_scales outputs, forward_fused_bias against forward_reference,
    next to two reference runs against each other: the yardstick of tests/test_gpu_decoder_fused.py."""
    net = _nets(1).train()
    x = torch.randn(2, 3, 128, 416, device=DEV, generator=torch.Generator(device=DEV).manual_seed(5))
    w = [torch.randn(2, 1, 128 // 2 ** s, 416 // 2 ** s, device=DEV,
                     generator=torch.Generator(device=DEV).manual_seed(10 + s)) for s in range(4)]

    def grads(new):
        net.zero_grad(set_to_none=True)
        feats = net.encoder(x)
        outs = net.decoder.forward_fused_bias(feats) if new else net.decoder.forward_reference(feats)
        sum((o * w[s]).sum() for s, o in enumerate(outs[:num_scales])).backward()
        return {n: p.grad.clone() for n, p in net.named_parameters() if p.grad is not None}

    ref1, ref2, got = grads(False), grads(False), grads(True)
    assert list(got) == list(ref1)
    worst_rel, worst_spread = 0.0, 0.0
    for n in got:
        g, r1, r2 = got[n], ref1[n], ref2[n]
        scale = float(r1.abs().max()) + 1e-30
        d = float((g - r1).abs().max())
        spread = float((r2 - r1).abs().max())
        worst_rel = max(worst_rel, d / scale)
        worst_spread = max(worst_spread, spread / scale)
        assert d <= 3 * spread + 1e-5 * scale, (n, tuple(g.shape), d, spread, scale)
    report(f"DispResNet gradients num_scales={num_scales}: folded biases vs reference worst {worst_rel:.2e} of scale, "
           f"reference vs reference {worst_spread:.2e}")


def test_a_captured_graph_replays_to_the_eager_result():
    """forward plus backward of the three ops (bias sums included: their workspaces come from torch.empty inside the
    capture and nothing synchronises) captured with torch.cuda.graph, replayed on new input contents."""
    from scsfm_hip import decoder_bias as DB
    gen = torch.Generator(device=DEV).manual_seed(9)
    a, skip = _rand(gen, 2, 5, 6, 131), _rand(gen, 2, 3, 12, 262)
    biases = [_rand(gen, 5).requires_grad_(), _rand(gen, 8).requires_grad_(), _rand(gen, 8).requires_grad_()]
    w = _rand(gen, 2, 8, 12, 262)
    a.requires_grad_()
    skip.requires_grad_()

    def step():
        p = DB.up_cat_pad(a, biases[0], skip)[:, :, 1:-1, 1:-1].contiguous()
        q = DB.elu_pad(p, biases[1])[:, :, 1:-1, 1:-1]
        out = DB.disp_head(q.contiguous(), biases[2], 10, 0.01)
        return (out,) + torch.autograd.grad((out * w).sum(), [a, skip] + biases)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    with torch.no_grad():
        a.copy_(_rand(gen, *a.shape))
        skip.copy_(_rand(gen, *skip.shape))
        for b in biases:
            b.copy_(_rand(gen, *b.shape))
    graph.replay()
    torch.cuda.synchronize()
    replayed = [t.clone() for t in captured]
    eager = step()
    graph.replay()
    torch.cuda.synchronize()
    for k, (r, e, c) in enumerate(zip(replayed, eager, captured)):
        assert same_bits(r, e) and same_bits(c, e), k
