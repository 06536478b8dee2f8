"""The backward of the decoder's full-resolution tail (scsfm_hip.decoder_dgrad, csrc_dgrad/scsfm_decoder_dgrad.hip) on
the GPU, at the shapes of tests/test_dgrad_hostsim.py and under its bound (tests/_dgrad_cases.py): against the ATen
chain in fp64 with its fp32 run as yardstick, exact inputs to the bit, impulses over coded weights, bit-identical
repeats, operands that are views between NaN, the autograd node against the three nodes it replaces, a child process for
torch's current stream and graph capture, one DispResNet forward and backward with the switch on and off, and smoke()'s
check."""
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest
import torch

import _dgrad_cases as DC
from _util import report

pytestmark = pytest.mark.gpu

DEV = "cuda"
_ids = ["x".join(map(str, s)) for s in DC.SHAPES]


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _tail(q, y, g_out, w, **kw):
    from scsfm_hip import decoder_dgrad as DG
    return DG.tail_bwd(_dev(q), _dev(y), _dev(g_out), _dev(w), DC.ALPHA, **kw)


@pytest.mark.parametrize("shape", DC.SHAPES, ids=_ids)
def test_tail_backward_against_the_aten_chain(shape):
    c = DC.case(shape)
    g, g_b, g_bias_b, g_bias_h = _tail(c["q"], c["y"], c["g_out"], c["w"])
    again = _tail(c["q"], c["y"], c["g_out"], c["w"])
    assert all(same_bits(a, b) for a, b in zip((g, g_b, g_bias_b, g_bias_h), again)), "a second call gives other bits"
    g0, g_b0, none_b, none_h = _tail(c["q"], c["y"], c["g_out"], c["w"], want_bias_b=False, want_bias_head=False)
    assert none_b is None and none_h is None and same_bits(g0, g) and same_bits(g_b0, g_b)
    y, go = _dev(c["y"]), _dev(c["g_out"])
    assert same_bits(g, ((go * DC.ALPHA) * (1 - y)) * y), "g is not disp_head_bwd_kernel's expression"
    worst = {}
    for name, got in (("g_b", g_b), ("g_bias_b", g_bias_b), ("g_bias_head", g_bias_h)):
        worst[name] = DC.ratio(got.cpu().numpy(), c["ref32"][name], c["ref64"][name], c["S"][name])
        assert worst[name] <= 1.0, (shape, name, worst[name])
    report(f"tail backward on the GPU {shape}: worst entry of g_b at {worst['g_b']:.3f}, of its bias sum at "
           f"{worst['g_bias_b']:.3f}, the head's bias at {worst['g_bias_head']:.3f} of the bound")


@pytest.mark.parametrize("shape", DC.SHAPES, ids=_ids)
def test_exact_inputs_and_impulses(shape):
    q, g_in, w = DC.exact_case(shape)
    g, g_b, g_bias_b, g_bias_h = _tail(q, None, g_in, w)
    want_b, want_bias_b, want_bias_h = DC.tail_ref64(q, g_in, w)
    assert np.array_equal(g.cpu().numpy(), g_in)
    got = g_b.cpu().numpy()
    assert np.array_equal(got.astype(np.float64), want_b), DC.first_difference(got, want_b)
    assert np.array_equal(g_bias_b.cpu().numpy().astype(np.float64), want_bias_b)
    assert np.array_equal(g_bias_h.cpu().numpy().astype(np.float64), want_bias_h)
    B, H, W = shape
    for pos in DC.impulse_positions(H, W):
        q, g_in, w = DC.impulse_case(shape, pos)
        got = _tail(q, None, g_in, w)[1].cpu().numpy()
        want_b = DC.tail_ref64(q, g_in, w)[0]
        assert np.array_equal(got.astype(np.float64), want_b), (pos, DC.first_difference(got, want_b))


@pytest.mark.parametrize("offset", [1, 1029])
def test_operands_that_are_views_between_nan(offset):
    """q, y, g_out and w as the allocator hands them out inside larger blocks: 4-byte aligned only, with NaN directly
    before and after.  A load outside an operand turns up as NaN."""
    from scsfm_hip import decoder_dgrad as DG
    c = DC.case((2, 17, 67), seed=offset)
    fresh = [_dev(c[k]) for k in ("q", "y", "g_out", "w")]
    want = DG.tail_bwd(*fresh, DC.ALPHA)

    def between_nan(t):
        flat = torch.full((offset + t.numel() + 1031,), float("nan"), device=DEV)
        v = flat[offset:offset + t.numel()].view(t.shape)
        v.copy_(t)
        assert v.is_contiguous() and v.data_ptr() % 16 != 0
        return flat, v

    placed = [between_nan(t) for t in fresh]
    got = DG.tail_bwd(*[v for _, v in placed], DC.ALPHA)
    assert all(bool(torch.isfinite(a).all()) and same_bits(a, b) for a, b in zip(got, want))
    for (flat, _), t in zip(placed, fresh):
        assert bool(torch.isnan(flat[:offset]).all()) and bool(torch.isnan(flat[offset + t.numel():]).all())
        assert same_bits(flat[offset:offset + t.numel()].view(t.shape), t)


def _leaves(shape, seed):
    B, H, W = shape
    gen = torch.Generator(device=DEV).manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, device=DEV, generator=gen)  # noqa: E731
    return [rnd(B, DC.C, H, W), rnd(DC.C), rnd(1, DC.C, 3, 3) / 12, rnd(1)], rnd(B, 1, H, W)


def test_head_tail_against_the_three_nodes_it_replaces():
    """forward bit-identical to elu_pad -> conv -> disp_head; gradients as close to that chain's as the bound's yardstick
    allows is checked above, here: the head's weight gradient to the bit (the same call on the same g), its bias gradient
    within an ulp (two fp64 sums of the same g in different orders, each rounded once), b's and its bias' gradient within
    1e-5 of scale; frozen inputs get no gradient and change no other"""
    from scsfm_hip import conv_wrw as CW, decoder_bias as DB, decoder_dgrad as DG
    leaves, gy = _leaves((2, 17, 67), 5)
    a = [t.clone().requires_grad_(True) for t in leaves]
    b = [t.clone().requires_grad_(True) for t in leaves]
    out = DG.head_tail(*a, DC.ALPHA, DC.BETA)
    ref = DB.disp_head(CW.conv3x3_valid(DB.elu_pad(b[0], b[1]), b[2]), b[3], DC.ALPHA, DC.BETA)
    assert same_bits(out, ref)
    got, want = torch.autograd.grad(out, a, gy), torch.autograd.grad(ref, b, gy)
    ulp = lambda a, b: float((a - b).abs().max()) <= 2.0 ** -23 * float(b.abs().max())  # noqa: E731
    assert ulp(got[3], want[3]) and same_bits(got[2], want[2])
    for k in (0, 1):
        assert float((got[k] - want[k]).abs().max()) <= 1e-5 * float(want[k].abs().max()), k
    for frozen in ((0,), (1,), (2,), (3,), (0, 1), (1, 3), (0, 1, 2), (0, 1, 3)):
        xs = [t.clone().requires_grad_(k not in frozen) for k, t in enumerate(leaves)]
        live = [k for k in range(4) if k not in frozen]
        gs = torch.autograd.grad(DG.head_tail(*xs, DC.ALPHA, DC.BETA), [xs[k] for k in live], gy)
        assert all(ulp(g, got[k]) if k == 3 else same_bits(g, got[k]) for g, k in zip(gs, live)), frozen


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "sc-sfmlearner-release_amd")

CHILD = textwrap.dedent("""
    import sys, torch
    sys.path.insert(0, %r)
    from scsfm_hip import conv_wrw as CW, decoder_dgrad as DG
    dev = torch.device("cuda:0")
    B, C, H, W = 6, 16, 33, 130
    bits = lambda a, b: a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))
    gen = torch.Generator(device=dev).manual_seed(11)
    rnd = lambda *s: torch.randn(*s, device=dev, generator=gen)
    q0, q1 = rnd(B, C, H + 2, W + 2), rnd(B, C, H + 2, W + 2)
    y0 = torch.sigmoid(rnd(B, 1, H, W))
    go0, go1 = rnd(B, 1, H, W), rnd(B, 1, H, W)
    w0 = rnd(1, C, 3, 3)
    gy0, gy1 = rnd(B, C, H, W), rnd(B, C, H, W)
    wc = rnd(C, C, 3, 3)

    def both(q, go, gy):  # the two new launches: the tail's backward and the 16 -> 16 data gradient
        return list(DG.tail_bwd(q, y0, go, w0, 10.0)) + [CW.data_grad(gy, wc)]

    eager0, eager1 = both(q0, go0, gy0), both(q1, go1, gy1)
    assert not bits(eager0[1], eager1[1]) and not bits(eager0[-1], eager1[-1])
    torch.cuda.synchronize()

    # the current stream: the operands are filled on a side stream, behind work that keeps that stream busy, and the
    # call follows with no host synchronisation; launched on another stream it would read the zeros
    q, go, gy = torch.zeros_like(q0), torch.zeros_like(go0), torch.zeros_like(gy0)
    busy = rnd(2048, 2048)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        for _ in range(8):
            busy = busy @ busy * 1e-3
        q.copy_(q0)
        go.copy_(go0)
        gy.copy_(gy0)
        got = both(q, go, gy)
    s.synchronize()
    assert all(bits(a, b) for a, b in zip(got, eager0)), "the launches do not follow torch's current stream"
    print("STREAM-OK")

    # graph capture of the tail's two launches and the data gradient's one (a linear graph), static inputs, warmed up
    # on a side stream
    qs, gos, gys = q0.clone(), go0.clone(), gy0.clone()

    def step():
        return both(qs, gos, gys)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step()
    graph.replay()
    torch.cuda.synchronize()
    first = [t.clone() for t in outs]
    with torch.no_grad():
        qs.copy_(q1)
        gos.copy_(go1)
        gys.copy_(gy1)
    graph.replay()
    torch.cuda.synchronize()
    second = [t.clone() for t in outs]
    assert all(bits(a, b) for a, b in zip(first, eager0)), "the first replay differs from the eager call"
    assert all(bits(a, b) for a, b in zip(second, eager1)), "the replay after an in-place update differs"
    print("GRAPH-OK")
""") % PKG


def test_current_stream_and_graph_capture():
    """decoder_dgrad.tail_bwd's and conv_wrw.data_grad's claims "launches go on torch's current stream" and "graph capture
    is safe", in a child process: a failure inside capture can take the interpreter down with it"""
    out = subprocess.run([sys.executable, "-c", CHILD], capture_output=True, text=True, timeout=300,
                         env=dict(os.environ, PYTHONPATH=PKG))
    assert out.returncode == 0 and "STREAM-OK" in out.stdout and "GRAPH-OK" in out.stdout, \
        out.stdout[-2000:] + out.stderr[-4000:]


def _disp_grads(net, x, on):
    from scsfm_hip import config
    config.set_decoder_dgrad(on)
    try:
        net.zero_grad(set_to_none=True)
        outs = net(x)
        sum((o * o).mean() for o in outs).backward()
        torch.cuda.synchronize()
        return [o.detach() for o in outs], {n: p.grad.clone() for n, p in net.named_parameters() if p.grad is not None}
    finally:
        config.set_decoder_dgrad(None)


@pytest.fixture
def deterministic_miopen():
    """as tests/test_gpu_decbias.py: MIOpen's default solvers for some of these shapes are not reproducible"""
    old = torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = True, False
    yield
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = old


def test_disp_resnet_with_the_switch_on_and_off(deterministic_miopen):
    """One DispResNet forward and backward at 2 x 3 x 64 x 96: the outputs keep their bits whenever the switched-off run
    reproduces itself; every parameter gradient is within 3 x the switched-off run's own repeat + 1e-5 x scale of it;
    switched on the kernel runs once, switched off not at all."""
    import models
    from scsfm_hip import decoder_dgrad as DG
    torch.manual_seed(0)
    net = models.DispResNet(18, False).to(DEV).train()
    x = torch.randn(2, 3, 64, 96, device=DEV)
    calls, real = [], DG.tail_bwd
    try:
        DG.tail_bwd = lambda *a, **k: calls.append(1) or real(*a, **k)
        out_on, g_on = _disp_grads(net, x, True)
        assert calls == [1]
        out_off, g_off = _disp_grads(net, x, False)
        assert calls == [1]
    finally:
        DG.tail_bwd = real
    out_off2, g_off2 = _disp_grads(net, x, False)
    reproducible = all(same_bits(a, b) for a, b in zip(out_off, out_off2))
    for s, (a, b, c) in enumerate(zip(out_on, out_off, out_off2)):
        if reproducible:
            assert same_bits(a, b), f"scale {s}"
        else:
            assert float((a - b).abs().max()) <= 3 * float((c - b).abs().max()), f"scale {s}"
    assert set(g_on) == set(g_off) == set(g_off2) and len(g_on) > 60
    worst = 0.0
    for name in g_on:
        scale = float(g_off[name].abs().max())
        d, own = float((g_on[name] - g_off[name]).abs().max()), float((g_off2[name] - g_off[name]).abs().max())
        assert d <= 3 * own + 1e-5 * scale, (name, d, own, scale)
        worst = max(worst, d / (scale + 1e-300))
    report(f"DispResNet 2x3x64x96, the tail's backward from libscsfm_dgrad.so: parameter gradients within {worst:.2e} of "
           f"their scale of the switched-off run; the switched-off forward reproducible {reproducible}")


def test_smoke_checks_the_library(capsys):
    """the part of smoke() that checks this library"""
    import inspect
    sys.path.insert(0, ROOT)
    import __graft_entry__ as G
    assert "_smoke_dgrad(dev)" in inspect.getsource(G.smoke)
    G._smoke_dgrad(torch.device("cuda:0"))
    assert "[smoke] dgrad: the tail's backward in one kernel" in capsys.readouterr().out
