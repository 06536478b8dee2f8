"""The weight-gradient kernels (csrc_wrw/scsfm_conv_wrw.hip) on the host simulator (tests/_hostsim_wrw.py), compiled
unchanged; tests/hostsim/wrw_shim.h supplies v_mfma_f32_16x16x4_f32 as the wave-cooperative k-ordered fmaf chain that
the instruction is, in its lane layout.

Every shape runs in both thread orders, twice (same bits), with two prefills of the output and the workspace (NaN and a
finite value), between NaN guard bands.  The shapes cover several Cin and Cout blocks and every (Cout, chunk)
instantiation, widths that are no multiple of 4 or of the 32-wide tile, a tile smaller than its halo, one tile for a
grid that would hold hundreds, and rows whose start is not 16-byte aligned.

Bound per entry:  |dW32 - dW64| <= 2 max|aten32 - dW64| + 8 u S,  with dW64 the fp64 autograd result, aten32 the CPU
fp32 result, S = sum |dy| |x| over the same terms in fp64 and u = 2^-24: the fmaf chain's measured error (3.5e-7 sum|a b| at
K = 4096, about 6 u) plus the final rounding.

In all of those a workgroup has one tile.  MULTI are the shapes at which it walks several, as it does in training (the
grid is capped at 512 workgroups over all Cin chunks): 17 x 67 is 3 x 3 tiles per image with rows 8, 8, 1 and widths 32,
32, 3, and 9 is coprime to every grid size, so a workgroup's successive tiles change between full, narrow, short and
corner in every combination and some workgroups walk one tile more than others.  Every (Cout, chunk) instantiation and
the head reach two tiles per workgroup, 114 x 16 -> 16 three.  A simulator call at these sizes takes 3 to 14 s, so they
run three times each (forward, reverse, the other prefill; same bits) and meet the same bound.

Beside the bound, which is loose by construction, two checks without a tolerance: inputs from {-1, 0, 1}, for which every
summation order is exact in fp32 as long as B H W < 2^24, must give the fp64 result to the bit (MULTI and two of SHAPES);
and one 1.0 in dy over an x of distinct integer codes must return exactly the 3 x 3 window of x under it, in the
impulse's row and nowhere else, for impulses on the tile corners and seams (tests/_wrw_cases.py)."""
import functools
import math

import numpy as np
import pytest
import torch

import _hostsim_wrw as HW
import _wrw_cases as WC
from _util import report

OTHER_FILL = 12345.0
U = 2.0 ** -24
# (B, Cin, Cout, H, W)
SHAPES = [(2, 16, 16, 5, 67), (1, 32, 16, 9, 130), (3, 96, 32, 6, 35), (2, 64, 32, 4, 4), (1, 16, 16, 1, 1),
          (2, 16, 32, 3, 5), (2, 16, 1, 7, 66), (1, 64, 1, 3, 33)]
# more tiles than workgroups: 9 B tiles over G = 512 / 512 / 512 / 256 / 170 / 512 / 512 workgroups
MULTI = [(58, 16, 16, 17, 67), (58, 32, 16, 17, 67), (58, 16, 32, 17, 67), (29, 64, 32, 17, 67), (20, 96, 32, 17, 67),
         (58, 16, 1, 17, 67), (114, 16, 16, 17, 67)]
EXACT = MULTI + [(2, 16, 16, 5, 67), (3, 96, 32, 6, 35)]
_ids = lambda shapes: ["x".join(map(str, s)) for s in shapes]


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
@pytest.mark.parametrize("shape", SHAPES, ids=_ids(SHAPES))
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


def _tiles(shape):
    """-> tiles per image, tiles, workgroups per chunk (from the library's own workspace size)"""
    B, Cin, Cout, H, W = shape
    per_image = -(-H // 8) * -(-W // 32)
    n = HW.ws_bytes(*shape)
    assert n > 0 and n % (4 * Cout * Cin * 9) == 0
    return per_image, B * per_image, n // 4 // (Cout * Cin * 9)


@pytest.mark.parametrize("shape", MULTI, ids=_ids(MULTI))
def test_several_tiles_per_workgroup_on_the_simulator(shape, monkeypatch):
    """the persistent loop beyond its first pass: prefetch(t + G) under the multiplication, a second commit over a used
    LDS tile, a tile extent carried from prefetch to commit"""
    x, dy, dw64, aten32, S = case(shape)
    _, ntiles, G = _tiles(shape)
    assert ntiles > G
    monkeypatch.delenv("HOSTSIM_ORDER", raising=False)
    got, ws = HW.conv3x3_wrw(x, dy)
    monkeypatch.setenv("HOSTSIM_ORDER", "reverse")
    rev, ws_rev = HW.conv3x3_wrw(x, dy)
    assert identical(got, rev) and identical(ws, ws_rev), "the thread order changes the result"
    monkeypatch.delenv("HOSTSIM_ORDER")
    other, ws_other = HW.conv3x3_wrw(x, dy, fill=OTHER_FILL)
    assert identical(got, other) and identical(ws, ws_other), "an output or workspace entry keeps its prefill"
    assert got.dtype == np.float32 and got.shape == dw64.shape and np.isfinite(got).all() and np.isfinite(ws).all()
    err = np.abs(got.astype(np.float64) - dw64)
    yard = np.abs(aten32.astype(np.float64) - dw64).max()
    bound = 2 * yard + 8 * U * S
    report(f"wrw on the simulator {shape}, {ntiles} tiles over {G} workgroups: max |dW32 - dW64| {err.max():.3e}, "
           f"aten32's {yard:.3e}, worst entry at {(err / bound).max():.3f} of its bound, at "
           f"{(err / (8 * U * S)).max():.3f} of 8 u S alone")
    assert np.all(err <= bound), (shape, float((err / bound).max()))


@pytest.mark.parametrize("shape", EXACT, ids=_ids(EXACT))
def test_ternary_inputs_give_the_fp64_result_exactly(shape):
    """zero tolerance: with x and dy from {-1, 0, 1} and B H W < 2^24 no sum the kernel forms is ever rounded"""
    B, _, _, H, W = shape
    assert B * H * W < 2 ** 24
    x, dy, dw64 = WC.ternary_case(shape)
    got, _ = HW.conv3x3_wrw(x.numpy(), dy.numpy())
    got = torch.from_numpy(got)
    wrong = int((got.double() != dw64).sum())
    report(f"wrw on the simulator {shape}, inputs from {{-1, 0, 1}}: max |dW| {float(dw64.abs().max()):.0f}, "
           f"{wrong} of {dw64.numel()} entries differ from fp64")
    assert torch.equal(got.double(), dw64), (shape, wrong, float((got.double() - dw64).abs().max()))


@pytest.mark.parametrize("pixel", WC.IMPULSE_PIXELS, ids=lambda p: f"h{p[0]}w{p[1]}")
@pytest.mark.parametrize("shape", WC.IMPULSE_SHAPES, ids=_ids(WC.IMPULSE_SHAPES))
def test_an_impulse_returns_the_window_of_x_under_it(shape, pixel):
    """the lane maps as the shim has them (the GPU's are checked by tests/test_gpu_wrw.py with the same impulses), the
    tile's origin and halo, and the (co, ci) block a wave owns: a wrong index returns another element's code"""
    B, _, Cout, _, _ = shape
    x = WC.impulse_x(shape)
    for co in WC.impulse_rows(Cout):
        dy = WC.impulse_dy(shape, B - 1, co, *pixel)
        got, _ = HW.conv3x3_wrw(x.numpy(), dy.numpy())
        failure = WC.impulse_failure(torch.from_numpy(got), x, shape, B - 1, co, *pixel)
        assert failure is None, failure


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
    # and MULTI is past it: every instantiation and a head with two tiles for some workgroup, one shape with three, no
    # shape whose workgroups all walk the same number, and a tile class that changes from one of a workgroup's tiles to
    # the next (the grid's size from the library, not from a copy of its constants)
    beyond = [s for s in MULTI if _tiles(s)[1] > _tiles(s)[2]]
    assert {(32 if cin >= 32 else 16, max(cout, 16)) for _, cin, cout, _, _ in beyond} == inst
    assert any(cout == 1 for _, _, cout, _, _ in beyond) and beyond == MULTI
    assert any(_tiles(s)[1] > 2 * _tiles(s)[2] for s in MULTI)
    assert all(_tiles(s)[1] % _tiles(s)[2] != 0 for s in MULTI)
    assert all(math.gcd(_tiles(s)[0], _tiles(s)[2]) == 1 for s in MULTI)
    assert all(h % 8 and w % 32 and h > 8 and w > 32 for *_, h, w in MULTI)       # full, narrow, short and corner tiles


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
