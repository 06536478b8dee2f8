"""The gradients of the encoders' 1x1 convolutions (scsfm_hip.conv1x1, csrc_pw/scsfm_pointwise.hip) on the GPU, at the
shapes of tests/_pw_cases.py: against ATen's fp64 result with its fp32 result (MIOpen's) beside it,

    per entry  |got - ref64| <= 2 max|ref32 - ref64| + 8 u S,     S the op on the absolute values in fp64, u = 2^-24

bit-identical repeats, exact zeros where the stride skips, operands from {-1, 0, 1} to the bit, operands that are views
between NaN at odd element offsets, the autograd function against F.conv2d's own node, the current stream and graph
capture in a child process, one ResNet-18 encoder forward and backward with the switch on and off, and smoke()'s check."""
import os
import subprocess
import sys
import textwrap

import pytest
import torch
import torch.nn.functional as F

import _pw_cases as PC
from _util import report

pytestmark = pytest.mark.gpu

DEV = "cuda"
ALL = PC.SHAPES + PC.MULTI


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize("shape", ALL, ids=PC.ids(ALL))
def test_weight_gradient_against_fp64_and_miopen(shape):
    from scsfm_hip import conv1x1 as PW
    B, Cin, Cout, H, W, s = shape
    x, dy, _ = PC.operands(shape, DEV)
    got = PW.weight_grad(x, dy, s)
    assert got.shape == (Cout, Cin, 1, 1) and got.dtype == torch.float32
    for _ in range(2):
        assert same_bits(got, PW.weight_grad(x, dy, s)), "a second call gives other bits"
    ref64, yard, S = PC.wgrad_refs(x, dy, s)
    ratio = PC.worst(got, ref64, yard, S)
    report(f"pw wrw on the GPU {shape}: MIOpen's max error {yard:.3e}, worst entry at {ratio:.3f} of its bound")
    assert ratio <= 1.0, (shape, ratio)
    xt, dyt, _ = PC.operands(shape, DEV, ternary=True)
    assert torch.equal(PW.weight_grad(xt, dyt, s).double(), PC.aten_wgrad(xt.double(), dyt.double(), s)), "ternary"


@pytest.mark.parametrize("shape", PC.DGRAD_SHAPES, ids=PC.ids(PC.DGRAD_SHAPES))
def test_data_gradient_against_fp64_and_miopen(shape):
    from scsfm_hip import conv1x1 as PW
    B, Cin, Cout, H, W, s = shape
    _, dy, w = PC.operands(shape, DEV)
    got = PW.data_grad(dy, w, H, W)
    assert got.shape == (B, Cin, H, W) and got.dtype == torch.float32
    for _ in range(2):
        assert same_bits(got, PW.data_grad(dy, w, H, W)), "a second call gives other bits"
    ref64, yard, S = PC.dgrad_refs(dy, w, H, W)
    ratio = PC.worst(got, ref64, yard, S)
    report(f"pw dgrad on the GPU {shape}: MIOpen's max error {yard:.3e}, worst entry at {ratio:.3f} of its bound")
    assert ratio <= 1.0, (shape, ratio)
    zeros = PC.unsampled(got)
    assert bool((zeros == 0).all()) and not bool(torch.signbit(zeros).any()), "a skipped position is not an exact +0"
    _, dyt, wt = PC.operands(shape, DEV, ternary=True)
    assert torch.equal(PW.data_grad(dyt, wt, H, W).double(), PC.aten_dgrad(dyt.double(), wt.double(), H, W)), "ternary"


@pytest.mark.parametrize("offset", [1, 1029])
@pytest.mark.parametrize("shape", [(5, 64, 128, 9, 67, 2), (1, 64, 128, 1, 1, 2), (2, 512, 256, 3, 7, 1)],
                         ids=lambda s: "x".join(map(str, s)))
def test_operands_that_are_views_between_nan(shape, offset):
    """x, dy, w and the outputs' surroundings as the allocator hands them out inside larger blocks: 4-byte aligned only,
    with NaN directly before and after.  A load outside an operand, even one that is then multiplied by zero, turns up
    as NaN."""
    from scsfm_hip import conv1x1 as PW
    B, Cin, Cout, H, W, s = shape
    x0, dy0, w0 = PC.operands(shape, DEV)
    want_w = PW.weight_grad(x0, dy0, s)
    want_x = PW.data_grad(dy0, w0, H, W) if s == 2 else None

    def between_nan(t):
        flat = torch.full((offset + t.numel() + 1031,), float("nan"), device=DEV)
        v = flat[offset:offset + t.numel()].view(t.shape)
        v.copy_(t)
        assert v.is_contiguous() and v.data_ptr() % 8 != 0 and v.data_ptr() == flat.data_ptr() + 4 * offset
        return flat, v

    (xf, x), (df, dy), (wf, w) = between_nan(x0), between_nan(dy0), between_nan(w0)
    got_w = PW.weight_grad(x, dy, s)
    assert bool(torch.isfinite(got_w).all()) and same_bits(got_w, want_w)
    if s == 2:
        got_x = PW.data_grad(dy, w, H, W)
        assert bool(torch.isfinite(got_x).all()) and same_bits(got_x, want_x)
    for flat, t in ((xf, x0), (df, dy0), (wf, w0)):      # and the calls left their operands and surroundings alone
        assert bool(torch.isnan(flat[:offset]).all()) and bool(torch.isnan(flat[offset + t.numel():]).all())
        assert same_bits(flat[offset:offset + t.numel()].view(t.shape), t)


@pytest.fixture
def deterministic_miopen():
    """as tests/test_gpu_wrw.py: MIOpen's default solvers for some of these shapes are not reproducible"""
    old = torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = True, False
    yield
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = old


@pytest.mark.parametrize("shape", [(3, 128, 256, 5, 35, 2), (2, 512, 256, 3, 7, 1)], ids=lambda s: "x".join(map(str, s)))
def test_conv1x1_against_the_convolutions_own_node(shape, deterministic_miopen, monkeypatch):
    """forward bit-identical to F.conv2d (two calls of MIOpen's forward: with its reproducible solvers), gradients under
    the bound, frozen inputs get no gradient and cost no launch"""
    from scsfm_hip import conv1x1 as PW
    B, Cin, Cout, H, W, s = shape
    monkeypatch.setattr(PW, "ROUTED", {(Cin, Cout, s)})
    monkeypatch.setattr(PW, "ROUTED_DGRAD", {(Cin, Cout, s)} if s == 2 else set())
    x0, gy, w0 = PC.operands(shape, DEV)
    bias = torch.randn(Cout, device=DEV).requires_grad_(True) if s == 1 else None  # (the pose decoder's squeeze has one)
    x, w = x0.clone().requires_grad_(True), w0.clone().requires_grad_(True)
    leaves = (x, w) + (() if bias is None else (bias,))
    y, y_ref = PW.conv1x1(x, w, bias, s), F.conv2d(x, w, bias, s)
    assert same_bits(y, y_ref)
    got, ref = torch.autograd.grad(y, leaves, gy), torch.autograd.grad(y_ref, leaves, gy)
    assert PC.worst(got[1], *PC.wgrad_refs(x0, gy, s)) <= 1.0
    assert same_bits(got[1], PW.weight_grad(x0, gy, s))
    if s == 2:
        assert PC.worst(got[0], *PC.dgrad_refs(gy, w0, H, W)) <= 1.0 and same_bits(got[0], PW.data_grad(gy, w0, H, W))
    else:
        assert float((got[0] - ref[0]).abs().max()) <= 1e-5 * float(ref[0].abs().max())  # (ATen's on both sides)
        assert float((got[2] - ref[2]).abs().max()) <= 1e-5 * float(ref[2].abs().max())
    calls = []
    real_w, real_d = PW.weight_grad, PW.data_grad
    monkeypatch.setattr(PW, "weight_grad", lambda *a: calls.append("w") or real_w(*a))
    monkeypatch.setattr(PW, "data_grad", lambda *a: calls.append("d") or real_d(*a))
    (gx2,) = torch.autograd.grad(PW.conv1x1(x, w.detach(), bias, s), (x,), gy)
    assert calls == (["d"] if s == 2 else []) and same_bits(gx2, got[0])
    del calls[:]
    (gw2,) = torch.autograd.grad(PW.conv1x1(x.detach(), w, bias, s), (w,), gy)
    assert calls == ["w"] and same_bits(gw2, got[1])
    y3 = PW.conv1x1(x.detach(), w.detach(), None, s)
    assert not y3.requires_grad


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "sc-sfmlearner-release_amd")

CHILD = textwrap.dedent("""
    import sys, torch
    sys.path.insert(0, %r)
    from scsfm_hip import conv1x1 as PW
    PW.ROUTED, PW.ROUTED_DGRAD = {(64, 128, 2)}, {(64, 128, 2)}
    dev = torch.device("cuda:0")
    B, Cin, Cout, H, W = 5, 64, 128, 9, 67
    bits = lambda a, b: a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))
    gen = torch.Generator(device=dev).manual_seed(11)
    rnd = lambda *s: torch.randn(*s, device=dev, generator=gen)
    x0, x1 = rnd(B, Cin, H, W), rnd(B, Cin, H, W)
    gy0, gy1 = rnd(B, Cout, 5, 34), rnd(B, Cout, 5, 34)
    w0 = rnd(Cout, Cin, 1, 1)
    eager = [(PW.weight_grad(x, gy, 2), PW.data_grad(gy, w0, H, W)) for x, gy in ((x0, gy0), (x1, gy1))]
    assert not bits(eager[0][0], eager[1][0]) and not bits(eager[0][1], eager[1][1])
    torch.cuda.synchronize()

    # the current stream: the operands are filled on a side stream, behind work that keeps that stream busy, and the
    # calls follow with no host synchronisation; launched on another stream they would read the zeros
    x, gy = torch.zeros_like(x0), torch.zeros_like(gy0)
    busy = rnd(2048, 2048)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        for _ in range(8):
            busy = busy @ busy * 1e-3
        x.copy_(x0)
        gy.copy_(gy0)
        got_w, got_x = PW.weight_grad(x, gy, 2), PW.data_grad(gy, w0, H, W)
    s.synchronize()
    assert bits(got_w, eager[0][0]) and bits(got_x, eager[0][1]), "the launches do not follow torch's current stream"
    print("STREAM-OK")

    # graph capture: one convolution's forward and backward (MIOpen's forward, then the library's three launches, a
    # linear graph), static inputs, warmed up on a side stream as torch documents
    xs, gys = x0.clone().requires_grad_(True), gy0.clone()
    w = w0.clone().requires_grad_(True)

    def step():
        return torch.autograd.grad(PW.conv1x1(xs, w, None, 2), (xs, w), gys)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        gx, gw = step()
    graph.replay()
    torch.cuda.synchronize()
    first = gx.clone(), gw.clone()
    with torch.no_grad():
        xs.copy_(x1)
        gys.copy_(gy1)
    graph.replay()
    torch.cuda.synchronize()
    second = gx.clone(), gw.clone()
    assert bits(first[1], eager[0][0]) and bits(first[0], eager[0][1]), "the first replay differs from the eager call"
    assert bits(second[1], eager[1][0]) and bits(second[0], eager[1][1]), "the replay after an update differs"
    print("GRAPH-OK")
""") % PKG


def test_current_stream_and_graph_capture():
    """conv1x1's claims "the launches go on torch's current stream" and "graph capture is safe", in a child process: a
    failure inside capture can take the interpreter down with it"""
    out = subprocess.run([sys.executable, "-c", CHILD], capture_output=True, text=True, timeout=300,
                         env=dict(os.environ, PYTHONPATH=PKG))
    assert out.returncode == 0 and "STREAM-OK" in out.stdout and "GRAPH-OK" in out.stdout, \
        out.stdout[-2000:] + out.stderr[-4000:]


def _encoder_grads(enc, x, on):
    from scsfm_hip import config
    config.set_conv1x1_bwd(on)
    try:
        enc.zero_grad(set_to_none=True)
        feats = enc(x)
        sum((f * f).mean() for f in feats).backward()
        torch.cuda.synchronize()
        return [f.detach() for f in feats], {n: p.grad.clone() for n, p in enc.named_parameters() if p.grad is not None}
    finally:
        config.set_conv1x1_bwd(None)


def test_resnet18_encoder_with_the_switch_on_and_off(deterministic_miopen, monkeypatch):
    """One ResNet-18 encoder forward and backward at 2 x 3 x 64 x 96 with every covered down-sample convolution routed:
    the features are bit-identical (the forward is the same call), every parameter gradient is within 3 x the
    switched-off run's own repeat plus 1e-5 of its scale; switched on, each of the three down-sample convolutions takes
    both gradients from the library once, switched off none does."""
    from models.resnet_encoder import ResnetEncoder
    from scsfm_hip import conv1x1 as PW
    triples ={(64, 128, 2), (128, 256, 2), (256, 512, 2)}
    monkeypatch.setattr(PW, "ROUTED", set(triples))
    monkeypatch.setattr(PW, "ROUTED_DGRAD", set(triples))
    torch.manual_seed(0)
    enc = ResnetEncoder(18, False).to(DEV).train()
    x = torch.randn(2, 3, 64, 96, device=DEV)
    calls = []
    real_w, real_d = PW.weight_grad, PW.data_grad
    monkeypatch.setattr(PW, "weight_grad", lambda a, b, s: calls.append(("w", a.shape[1], b.shape[1], s)) or real_w(a, b, s))
    monkeypatch.setattr(PW, "data_grad", lambda g, w, *hw: calls.append(("d", w.shape[1], w.shape[0], 2)) or real_d(g, w, *hw))
    f_on, g_on = _encoder_grads(enc, x, True)
    assert sorted(calls) == sorted([(k,) + t for k in "dw" for t in triples])
    del calls[:]
    f_off, g_off = _encoder_grads(enc, x, False)
    f_off2, g_off2 = _encoder_grads(enc, x, False)
    assert not calls
    for level, (a, b) in enumerate(zip(f_on, f_off)):
        assert same_bits(a, b), f"feature {level}"
    assert set(g_on) == set(g_off) == set(g_off2)
    worst = 0.0
    for name in g_on:
        scale = float(g_off[name].abs().max())
        d, own = float((g_on[name] - g_off[name]).abs().max()), float((g_off2[name] - g_off[name]).abs().max())
        assert d <= 3 * own + 1e-5 * scale, (name, d, own, scale)
        worst = max(worst, d / scale if scale else 0.0)
    report(f"ResNet-18 encoder 2x3x64x96, the down-sample convolutions' gradients from libscsfm_pw.so: largest parameter-"
           f"gradient difference to the switched-off run {worst:.2e} of the gradient's scale")


def test_smoke_checks_the_library(capsys):
    """the part of smoke() that checks this library (smoke() calls it last)"""
    import inspect
    sys.path.insert(0, ROOT)
    import __graft_entry__ as G
    assert "_smoke_pw(dev)" in inspect.getsource(G.smoke)
    G._smoke_pw(torch.device("cuda:0"))
    assert "[smoke] pw: weight gradient of a 64 -> 128 stride-2 1x1 convolution" in capsys.readouterr().out
