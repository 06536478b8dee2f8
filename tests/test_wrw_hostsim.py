"""The weight-gradient kernels (csrc_wrw/scsfm_conv_wrw.hip) on the host simulator (tests/_hostsim_wrw.py), compiled
unchanged; tests/hostsim/wrw_shim.h supplies v_mfma_f32_16x16x4_f32 as the wave-cooperative k-ordered fmaf chain that
the instruction is, in its lane layout.

Every shape runs in both thread orders, twice (same bits), with two prefills of the output and the workspace (NaN and a
finite value), between NaN guard bands.  The shapes cover several Cin and Cout blocks and every (Cout, chunk)
instantiation, widths that are no multiple of 4 or of the 32-wide tile, a tile smaller than its halo, one tile for a
grid that would hold hundreds, and rows whose start is not 16-byte aligned.

Bound per entry:  |dW32 - dW64| <= 2 max|aten32 - dW64| + 8 u S,  with dW64 the fp64 autograd result, aten32 the CPU
fp32 result, S = sum |dy| |x| over the same terms in fp64 and u = 2^-24: the fmaf chain's measured error (3.5e-7 sum|a b| at
K = 4096, about 6 u) plus the final rounding."""
import functools

import numpy as np
import pytest
import torch

import _hostsim_wrw as HW
from _util import report

OTHER_FILL = 12345.0
U = 2.0 ** -24
# (B, Cin, Cout, H, W)
SHAPES = [(2, 16, 16, 5, 67), (1, 32, 16, 9, 130), (3, 96, 32, 6, 35), (2, 64, 32, 4, 4), (1, 16, 16, 1, 1),
          (2, 16, 32, 3, 5), (2, 16, 1, 7, 66), (1, 64, 1, 3, 33)]


def _wgrad(x, dy):
    w = torch.zeros(dy.shape[1], x.shape[1], 3, 3, dtype=x.dtype)
    return torch.ops.aten.convolution_backward(dy, x, w, None, [1, 1], [0, 0], [1, 1], False, [0, 0], 1,
                                               [False, True, False])[1]


@functools.lru_cache(maxsize=None)
def case(shape):
    """x, dy (fp32 numpy) and the three references of a shape, computed once"""
    B, Cin, Cout, H, W = shape
    g = torch.Generator().manual_seed(1000 * Cin + 10 * H + W)
    x = torch.randn(B, Cin, H + 2, W + 2, generator=g)
    dy = torch.randn(B, Cout, H, W, generator=g)
    dw64 = _wgrad(x.double(), dy.double())
    aten32 = _wgrad(x, dy)
    S = _wgrad(x.double().abs(), dy.double().abs())
    out = tuple(t.numpy() for t in (x, dy, dw64, aten32, S))
    for a in out:
        a.setflags(write=False)
    return out


def identical(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


@pytest.mark.parametrize("order", ["forward", "reverse"])
@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_weight_gradient_on_the_simulator(shape, order, monkeypatch):
    x, dy, dw64, aten32, S = case(shape)
    monkeypatch.delenv("HOSTSIM_ORDER", raising=False)
    first, ws_first = HW.conv3x3_wrw(x, dy)
    if order == "reverse":
        monkeypatch.setenv("HOSTSIM_ORDER", "reverse")
        got, ws = HW.conv3x3_wrw(x, dy)
        assert identical(first, got) and identical(ws_first, ws), "the thread order changes the result"
    else:
        got, ws = first, ws_first
    again, ws_again = HW.conv3x3_wrw(x, dy)
    assert identical(got, again) and identical(ws, ws_again), "a second call gives other bits"
    other, ws_other = HW.conv3x3_wrw(x, dy, fill=OTHER_FILL)
    assert identical(got, other) and identical(ws, ws_other), "an output or workspace entry keeps its prefill"
    assert got.dtype == np.float32 and got.shape == dw64.shape and np.isfinite(got).all() and np.isfinite(ws).all()
    err = np.abs(got.astype(np.float64) - dw64)
    yard = np.abs(aten32.astype(np.float64) - dw64).max()
    bound = 2 * yard + 8 * U * S
    report(f"wrw on the simulator {shape} {order}: max |dW32 - dW64| {err.max():.3e}, aten32's {yard:.3e}, "
           f"worst entry at {(err / bound).max():.3f} of its bound, at {(err / (8 * U * S)).max():.3f} of 8 u S alone")
    assert np.all(err <= bound), (shape, float((err / bound).max()))


def test_the_shapes_cover_what_the_kernel_distinguishes():
    lib = HW.lib()
    inst = {(32 if cin >= 32 else 16, max(cout, 16)) for _, cin, cout, _, _ in SHAPES}
    assert inst == {(16, 16), (32, 16), (32, 32), (16, 32)}                       # every (chunk, Cout) instantiation
    assert any(cout == 1 for _, _, cout, _, _ in SHAPES)                           # a head: one row of a 16-row block
    assert {cin // 32 for _, cin, _, _, _ in SHAPES if cin >= 32} >= {1, 2, 3}     # one, two and three chunks
    assert any(w % 4 and w % 32 and w > 32 for *_, w in SHAPES)                    # no multiple of 4 or of the tile
    assert any(h > 8 for *_, h, _ in SHAPES) and any(h < 2 and w < 2 for *_, h, w in SHAPES)
    assert any((w + 2) % 4 for *_, w in SHAPES)                                    # rows that are not 16-byte aligned
    # a shape's grid is its tile count when that is below the 512 slots
    assert lib.size("scsfm_wrw_conv3x3_ws_bytes", 1, 16, 16, 1, 1) == 4 * 16 * 16 * 9
    assert lib.size("scsfm_wrw_conv3x3_ws_bytes", 1, 32, 16, 9, 130) == 4 * 10 * 16 * 32 * 9


def test_rejected_arguments_write_nothing():
    x, dy, *_ = case((2, 64, 32, 4, 4))
    k = HW._Call()
    xa, dya = k.arg(x), k.arg(dy)
    n = HW.ws_bytes(2, 64, 32, 4, 4)
    dw, ws = k.out((32, 64, 3, 3), np.nan), k.out((n // 4,), np.nan)
    p = HW._ptr
    for args in ((2, 64, 32, 4, 4, p(xa), p(dya), p(dw), p(ws), n - 4, None),
                 (2, 48, 32, 4, 4, p(xa), p(dya), p(dw), p(ws), n, None),
                 (2, 64, 32, 4, 4, None, p(dya), p(dw), p(ws), n, None),
                 (2, 64, 32, 4, 4, p(xa), p(dya), p(dw), None, n, None)):
        k.run("scsfm_wrw_conv3x3_f32", *args, status=-1)
    assert np.isnan(dw).all() and np.isnan(ws).all()
