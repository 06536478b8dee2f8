"""The weight gradient of the decoder's low-channel convolutions (scsfm_hip.conv_wrw, csrc_wrw/scsfm_conv_wrw.hip) on
the GPU, at the shapes of tests/test_wrw_hostsim.py: against the fp64 result with MIOpen's fp32 result beside it,

    per entry  |dW32 - dW64| <= 2 max|miopen32 - dW64| + 8 u S,     S = sum |dy| |x| in fp64, u = 2^-24

(the bound of tests/test_wrw_hostsim.py with MIOpen's weight gradient as the fp32 yardstick), bit-identical repeats, the
autograd function against F.conv2d's own node, one DispResNet forward and backward with the switch on and off, and
smoke()'s check of one shape.

In SHAPES a workgroup has one tile.  MULTI are the shapes of tests/test_wrw_hostsim.py's MULTI with the batch raised
until every (Cout, chunk) instantiation and the head walk three tiles per workgroup (9 B tiles of 17 x 67 over 512, 256
or 170 workgroups; the largest input is 19 MB): the same bound, and beside it the checks without a tolerance of
tests/_wrw_cases.py.  Inputs from {-1, 0, 1} must give the fp64 result to the bit (MIOpen's fp32 result is reported
beside it, not judged).  An impulse in dy over an x of distinct integer codes must return the 3 x 3 window under it and
zero elsewhere, which confirms on the real matrix instruction the lane maps that the simulator's shim assumes and says
which element a wrong map multiplied.  Operands that are views into NaN-filled buffers at offsets of 1 and of 1029 floats
(not 16-byte aligned, NaN directly before and after) must give the bits of freshly allocated copies.  A child process
checks that the launches follow torch's current stream and that a captured graph of one convolution's forward and
backward replays to the eager bits and follows inputs updated in place."""
import os
import subprocess
import sys
import textwrap

import pytest
import torch
import torch.nn.functional as F

import _wrw_cases as WC
from _util import report

pytestmark = pytest.mark.gpu

DEV = "cuda"
U = 2.0 ** -24
# (B, Cin, Cout, H, W)
SHAPES = [(2, 16, 16, 5, 67), (1, 32, 16, 9, 130), (3, 96, 32, 6, 35), (2, 64, 32, 4, 4), (1, 16, 16, 1, 1),
          (2, 16, 32, 3, 5), (2, 16, 1, 7, 66), (1, 64, 1, 3, 33)]
# three tiles for some workgroups: 1026 tiles over 512 workgroups, 522 over 256, 342 over 170
MULTI = [(114, 16, 16, 17, 67), (114, 32, 16, 17, 67), (114, 16, 32, 17, 67), (58, 64, 32, 17, 67),
         (38, 96, 32, 17, 67), (114, 16, 1, 17, 67)]
EXACT = MULTI + [(2, 16, 16, 5, 67), (3, 96, 32, 6, 35)]
_ids = lambda shapes: ["x".join(map(str, s)) for s in shapes]


def _wgrad(x, dy):
    w = torch.zeros(dy.shape[1], x.shape[1], 3, 3, dtype=x.dtype, device=x.device)
    return torch.ops.aten.convolution_backward(dy, x, w, None, [1, 1], [0, 0], [1, 1], False, [0, 0], 1,
                                               [False, True, False])[1]


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _grid(shape):
    """-> tiles, workgroups per chunk (from the library's own workspace size)"""
    from scsfm_hip import _lib
    B, Cin, Cout, H, W = shape
    n = _lib.get_wrw().size("scsfm_wrw_conv3x3_ws_bytes", *shape)
    assert n > 0 and n % (4 * Cout * Cin * 9) == 0
    return B * -(-H // 8) * -(-W // 32), n // 4 // (Cout * Cin * 9)


@pytest.mark.parametrize("shape", SHAPES + MULTI, ids=_ids(SHAPES + MULTI))
def test_weight_gradient_against_fp64_and_miopen(shape):
    from scsfm_hip import conv_wrw as CW
    ntiles, G = _grid(shape)
    assert (ntiles > 2 * G) == (shape in MULTI)
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
    report(f"wrw on the GPU {shape}, {ntiles} tiles over {G} workgroups: max |dW32 - dW64| {float(err.max()):.3e}, MIOpen's {yard:.3e}, worst entry at "
           f"{float((err / bound).max()):.3f} of its bound, at {float((err / (8 * U * S)).max()):.3f} of 8 u S alone")
    assert bool((err <= bound).all()), (shape, float((err / bound).max()))


@pytest.mark.parametrize("shape", EXACT, ids=_ids(EXACT))
def test_ternary_inputs_give_the_fp64_result_exactly(shape):
    """zero tolerance: with x and dy from {-1, 0, 1} and B H W < 2^24 no sum the kernel forms is ever rounded"""
    from scsfm_hip import conv_wrw as CW
    B, _, _, H, W = shape
    assert B * H * W < 2 ** 24
    x, dy, dw64 = WC.ternary_case(shape, DEV)
    got = CW.weight_grad(x, dy)
    wrong, miopen_wrong = int((got.double() != dw64).sum()), int((_wgrad(x, dy).double() != dw64).sum())
    report(f"wrw on the GPU {shape}, inputs from {{-1, 0, 1}}: max |dW| {float(dw64.abs().max()):.0f}, {wrong} of "
           f"{dw64.numel()} entries differ from fp64 (MIOpen's fp32 gradient: {miopen_wrong})")
    assert torch.equal(got.double(), dw64), (shape, wrong, float((got.double() - dw64).abs().max()))


@pytest.mark.parametrize("pixel", WC.IMPULSE_PIXELS, ids=lambda p: f"h{p[0]}w{p[1]}")
@pytest.mark.parametrize("shape", WC.IMPULSE_SHAPES, ids=_ids(WC.IMPULSE_SHAPES))
def test_an_impulse_returns_the_window_of_x_under_it(shape, pixel):
    """the A, B and C/D lane maps of v_mfma_f32_16x16x4_f32 as the kernel uses them ("nothing is transposed"), the tile's
    origin and halo, and the (co, ci) block a wave owns: a wrong index returns another element's code, and the message
    says whose"""
    from scsfm_hip import conv_wrw as CW
    B, _, Cout, _, _ = shape
    x = WC.impulse_x(shape, DEV)
    x_cpu = x.cpu()
    for co in WC.impulse_rows(Cout):
        got = CW.weight_grad(x, WC.impulse_dy(shape, B - 1, co, *pixel, device=DEV))
        failure = WC.impulse_failure(got.cpu(), x_cpu, shape, B - 1, co, *pixel)
        assert failure is None, failure


@pytest.mark.parametrize("offset", [1, 1029])
@pytest.mark.parametrize("shape", [(58, 64, 32, 17, 67), (1, 16, 16, 1, 1)], ids=lambda s: "x".join(map(str, s)))
def test_operands_that_are_views_between_nan(shape, offset):
    """x and dy as the allocator hands them out inside larger blocks: 4-byte aligned only, with NaN directly before and
    after.  A load outside an operand, even one that is then multiplied by zero, turns up as NaN."""
    from scsfm_hip import conv_wrw as CW
    B, Cin, Cout, H, W = shape
    gen = torch.Generator(device=DEV).manual_seed(offset)
    x0 = torch.randn(B, Cin, H + 2, W + 2, device=DEV, generator=gen)
    dy0 = torch.randn(B, Cout, H, W, device=DEV, generator=gen)
    want = CW.weight_grad(x0, dy0)

    def between_nan(t):
        flat = torch.full((offset + t.numel() + 1031,), float("nan"), device=DEV)
        v = flat[offset:offset + t.numel()].view(t.shape)
        v.copy_(t)
        assert v.is_contiguous() and v.data_ptr() % 16 != 0 and v.data_ptr() == flat.data_ptr() + 4 * offset
        return flat, v

    xf, x = between_nan(x0)
    df, dy = between_nan(dy0)
    got = CW.weight_grad(x, dy)
    assert bool(torch.isfinite(got).all()) and same_bits(got, want)
    for flat, t in ((xf, x0), (df, dy0)):      # and the call left its operands and their surroundings alone
        assert bool(torch.isnan(flat[:offset]).all()) and bool(torch.isnan(flat[offset + t.numel():]).all())
        assert same_bits(flat[offset:offset + t.numel()].view(t.shape), t)


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "sc-sfmlearner-release_amd")

CHILD = textwrap.dedent("""
    import sys, torch
    sys.path.insert(0, %r)
    from scsfm_hip import conv_wrw as CW
    dev = torch.device("cuda:0")
    B, Cin, Cout, H, W = 58, 32, 16, 17, 67
    bits = lambda a, b: a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))
    gen = torch.Generator(device=dev).manual_seed(11)
    rnd = lambda *s: torch.randn(*s, device=dev, generator=gen)
    x0, x1 = rnd(B, Cin, H + 2, W + 2), rnd(B, Cin, H + 2, W + 2)
    gy0, gy1 = rnd(B, Cout, H, W), rnd(B, Cout, H, W)
    w0 = rnd(Cout, Cin, 3, 3)
    eager0, eager1 = CW.weight_grad(x0, gy0), CW.weight_grad(x1, gy1)
    assert not bits(eager0, eager1)
    torch.cuda.synchronize()

    # the current stream: the operands are filled on a side stream, behind work that keeps that stream busy, and the
    # call follows with no host synchronisation; launched on another stream it would read the zeros
    x, gy = torch.zeros_like(x0), torch.zeros_like(gy0)
    busy = rnd(2048, 2048)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        for _ in range(8):
            busy = busy @ busy * 1e-3
        x.copy_(x0)
        gy.copy_(gy0)
        got = CW.weight_grad(x, gy)
    s.synchronize()
    assert bits(got, eager0), "the launches do not follow torch's current stream"
    print("STREAM-OK")

    # graph capture: one convolution's forward and backward (the weight gradient alone: the kernel's two launches after
    # MIOpen's forward, a linear graph), static inputs, warmed up on a side stream as torch documents
    xs, gys = x0.clone(), gy0.clone()
    w = w0.clone().requires_grad_(True)

    def step():
        return torch.autograd.grad(CW.conv3x3_valid(xs, w), (w,), gys)[0]

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        gw = step()
    graph.replay()
    torch.cuda.synchronize()
    first = gw.clone()
    with torch.no_grad():
        xs.copy_(x1)
        gys.copy_(gy1)
    graph.replay()
    torch.cuda.synchronize()
    second = gw.clone()
    assert bits(first, eager0), "the first replay differs from the eager call"
    assert bits(second, eager1), "the replay after an in-place update differs from the eager call"
    assert not bits(first, second)
    print("GRAPH-OK")
""") % PKG


def test_current_stream_and_graph_capture():
    """conv_wrw's claims "the launches go on torch's current stream" and "graph capture is safe", in a child process: a
    failure inside capture can take the interpreter down with it"""
    out = subprocess.run([sys.executable, "-c", CHILD], capture_output=True, text=True, timeout=300,
                         env=dict(os.environ, PYTHONPATH=PKG))
    assert out.returncode == 0 and "STREAM-OK" in out.stdout and "GRAPH-OK" in out.stdout, \
        out.stdout[-2000:] + out.stderr[-4000:]


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
