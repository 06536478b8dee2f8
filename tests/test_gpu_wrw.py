"""The weight gradient of the decoder's low-channel convolutions (scsfm_hip.conv_wrw, csrc_wrw/scsfm_conv_wrw.hip) on
the GPU, at the shapes of tests/test_wrw_hostsim.py: against the fp64 result with MIOpen's fp32 result beside it,

    per entry  |dW32 - dW64| <= 2 max|miopen32 - dW64| + 8 u S,     S = sum |dy| |x| in fp64, u = 2^-24

(the bound of tests/test_wrw_hostsim.py with MIOpen's weight gradient as the fp32 yardstick), bit-identical repeats, the
autograd function against F.conv2d's own node, one DispResNet forward and backward with the switch on and off, and
smoke()'s check of one shape."""
import pytest
import torch
import torch.nn.functional as F

from _util import report

pytestmark = pytest.mark.gpu

DEV = "cuda"
U = 2.0 ** -24
# (B, Cin, Cout, H, W)
SHAPES = [(2, 16, 16, 5, 67), (1, 32, 16, 9, 130), (3, 96, 32, 6, 35), (2, 64, 32, 4, 4), (1, 16, 16, 1, 1),
          (2, 16, 32, 3, 5), (2, 16, 1, 7, 66), (1, 64, 1, 3, 33)]


def _wgrad(x, dy):
    w = torch.zeros(dy.shape[1], x.shape[1], 3, 3, dtype=x.dtype, device=x.device)
    return torch.ops.aten.convolution_backward(dy, x, w, None, [1, 1], [0, 0], [1, 1], False, [0, 0], 1,
                                               [False, True, False])[1]


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_weight_gradient_against_fp64_and_miopen(shape):
    from scsfm_hip import conv_wrw as CW
    B, Cin, Cout, H, W = shape
    gen = torch.Generator(device=DEV).manual_seed(1000 * Cin + 10 * H + W)
    x = torch.randn(B, Cin, H + 2, W + 2, device=DEV, generator=gen)
    dy = torch.randn(B, Cout, H, W, device=DEV, generator=gen)
    got = CW.weight_grad(x, dy)
    assert got.shape == (Cout, Cin, 3, 3) and got.dtype == torch.float32
    for _ in range(2):
        assert same_bits(got, CW.weight_grad(x, dy)), "a second call gives other bits"
    dw64, miopen32 = _wgrad(x.double(), dy.double()), _wgrad(x, dy)
    S = _wgrad(x.double().abs(), dy.double().abs())
    err, yard = (got.double() - dw64).abs(), float((miopen32.double() - dw64).abs().max())
    bound = 2 * yard + 8 * U * S
    report(f"wrw on the GPU {shape}: max |dW32 - dW64| {float(err.max()):.3e}, MIOpen's {yard:.3e}, worst entry at "
           f"{float((err / bound).max()):.3f} of its bound, at {float((err / (8 * U * S)).max()):.3f} of 8 u S alone")
    assert bool((err <= bound).all()), (shape, float((err / bound).max()))


def test_conv3x3_valid_against_the_convolutions_own_node():
    """forward bit-identical to F.conv2d, the input gradient MIOpen's data gradient, a frozen weight costs no launch"""
    from scsfm_hip import conv_wrw as CW
    gen = torch.Generator(device=DEV).manual_seed(3)
    x = torch.randn(2, 32, 11, 37, device=DEV, generator=gen, requires_grad=True)
    w = torch.randn(16, 32, 3, 3, device=DEV, generator=gen, requires_grad=True)
    gy = torch.randn(2, 16, 9, 35, device=DEV, generator=gen)
    y, y_ref = CW.conv3x3_valid(x, w), F.conv2d(x, w)
    assert same_bits(y, y_ref)
    gx, gw = torch.autograd.grad(y, (x, w), gy)
    gx_ref, gw_ref = torch.autograd.grad(y_ref, (x, w), gy)
    assert float((gx - gx_ref).abs().max()) <= 1e-5 * float(gx_ref.abs().max())
    assert same_bits(gw, CW.weight_grad(x.detach(), gy))
    assert float((gw - gw_ref).abs().max()) <= 1e-4 * float(gw_ref.abs().max())
    calls = []
    real = CW.weight_grad
    try:
        CW.weight_grad = lambda *a: calls.append(1) or real(*a)
        w_frozen = w.detach()
        (gx2,) = torch.autograd.grad(CW.conv3x3_valid(x, w_frozen), (x,), gy)
        assert not calls and same_bits(gx2, gx)
        x_frozen = x.detach()
        (gw2,) = torch.autograd.grad(CW.conv3x3_valid(x_frozen, w), (w,), gy)
        assert calls == [1] and same_bits(gw2, gw)
    finally:
        CW.weight_grad = real


def _disp_grads(net, x, on):
    from scsfm_hip import config
    config.set_decoder_wrw(on)
    try:
        net.zero_grad(set_to_none=True)
        outs = net(x)
        sum((o * o).mean() for o in outs).backward()
        torch.cuda.synchronize()
        return [o.detach() for o in outs], {n: p.grad.clone() for n, p in net.named_parameters() if p.grad is not None}
    finally:
        config.set_decoder_wrw(None)


@pytest.fixture
def deterministic_miopen():
    """as tests/test_gpu_decbias.py: MIOpen's default solvers for some of these shapes are not reproducible"""
    old = torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = True, False
    yield
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = old


def test_disp_resnet_with_the_switch_on_and_off(deterministic_miopen):
    """One DispResNet forward and backward at 2 x 3 x 64 x 96: the outputs (the forward is the same) are bit-identical
    whenever the switched-off run reproduces itself, otherwise no further apart than 3 x two runs of it; every routed
    layer took the kernel once and its weight gradient meets the bound of this file on the tensors the
    backward handed it; every other parameter gradient is as close to the switched-off run as that run's own repeat
    (MIOpen's weight gradients are atomic sums); switched off, the kernel is not called."""
    import models
    from scsfm_hip import conv_wrw as CW
    torch.manual_seed(0)
    net = models.DispResNet(18, False).to(DEV).train()
    x = torch.randn(2, 3, 64, 96, device=DEV)
    calls, worst = [], [0.0]
    real = CW.weight_grad

    def checked(a, b):
        got = real(a, b)
        dw64, S = _wgrad(a.double(), b.double()), _wgrad(a.double().abs(), b.double().abs())
        yard = float((_wgrad(a, b).double() - dw64).abs().max())
        ratio = float(((got.double() - dw64).abs() / (2 * yard + 8 * U * S)).max())
        assert ratio <= 1.0, ((a.shape[1], b.shape[1]), ratio)
        worst[0] = max(worst[0], ratio)
        calls.append((a.shape[1], b.shape[1]))
        return got

    try:
        CW.weight_grad = checked
        out_on, g_on = _disp_grads(net, x, True)
        n_on = len(calls)
        out_off, g_off = _disp_grads(net, x, False)
        assert len(calls) == n_on
    finally:
        CW.weight_grad = real
    out_off2, g_off2 = _disp_grads(net, x, False)
    assert set(calls) == CW.ROUTED and n_on == len(CW.ROUTED)
    reproducible = all(same_bits(a, b) for a, b in zip(out_off, out_off2))
    for s, (a, b, c) in enumerate(zip(out_on, out_off, out_off2)):
        if reproducible:
            assert same_bits(a, b), f"scale {s}"
        else:
            assert float((a - b).abs().max()) <= 3 * float((c - b).abs().max()), f"scale {s}"
    routed = {n for n, p in net.named_parameters() if p.dim() == 4 and tuple(p.shape[2:]) == (3, 3)
              and n.startswith("decoder.") and (p.shape[1], p.shape[0]) in CW.ROUTED}
    assert len(routed) == len(CW.ROUTED) and routed <= set(g_on) and set(g_on) == set(g_off) == set(g_off2)
    for name in g_on:
        if name in routed:
            continue
        scale = float(g_off[name].abs().max())
        d, own = float((g_on[name] - g_off[name]).abs().max()), float((g_off2[name] - g_off[name]).abs().max())
        assert d <= 3 * own + 1e-6 * scale, (name, d, own, scale)
    report(f"DispResNet 2x3x64x96, the routed layers' weight gradients from libscsfm_wrw.so: worst entry at "
           f"{worst[0]:.3f} of its bound; the switched-off forward reproducible {reproducible}")


def test_smoke_checks_the_library(capsys):
    """the part of smoke() that checks this library (smoke() calls it last)"""
    import inspect
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import __graft_entry__ as G
    assert "_smoke_wrw(dev)" in inspect.getsource(G.smoke)
    G._smoke_wrw(torch.device("cuda:0"))
    assert "[smoke] wrw: weight gradient of a 16 -> 16 convolution" in capsys.readouterr().out
