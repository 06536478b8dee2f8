"""The tail-backward kernel (csrc_dgrad/scsfm_decoder_dgrad.hip) on the host simulator (tests/_hostsim_dgrad.py), at the
shapes of tests/_dgrad_cases.py: (1, 2, 2) where every pixel is a corner, odd sizes, and sizes with several 8 x 64
tiles, partial ones included.

g_b and both bias sums against the ATen chain in fp64 with its fp32 run as yardstick (the bound of
tests/_dgrad_cases.py); g bit for bit ((g_out * alpha) * (1 - y)) * y in fp32; in null-y mode inputs whose arithmetic is
exact must give the fp64 result to the bit, and impulses of g over weights of distinct codes must return the flipped
3 x 3 window with its reflection folds; a frozen bias writes nothing; bad arguments return SCSFM_ERR_ARG and write
nothing.  Every case runs twice (same bits), in both thread orders, with two prefills of the outputs and the workspace,
between NaN guard bands."""
import ctypes

import numpy as np
import pytest

import _dgrad_cases as DC
import _hostsim_dgrad as HD
from _util import report

OTHER_FILL = 12345.0
_ids = ["x".join(map(str, s)) for s in DC.SHAPES]


def identical(xs, ys):
    assert len(xs) == len(ys)
    return all((x is None and y is None) or
               (x.shape == y.shape and np.array_equal(x.view(np.uint8), y.view(np.uint8))) for x, y in zip(xs, ys))


def both_orders_and_fills(run, order, monkeypatch):
    """run(fill) -> tuple of arrays; the NaN-prefilled results in the asked thread order, after checking that a second
    call, the other order and the other prefill give the same bits"""
    monkeypatch.delenv("HOSTSIM_ORDER", raising=False)
    first = run(np.nan)
    if order == "reverse":
        monkeypatch.setenv("HOSTSIM_ORDER", "reverse")
        got = run(np.nan)
        assert identical(first, got), "the thread order changes the result"
    else:
        got = first
    assert identical(got, run(np.nan)), "a second call gives other bits"
    assert identical(got, run(OTHER_FILL)), "an output entry keeps its prefill"
    return got


def ws_untouched(ws, fill):
    return np.isnan(ws).all() if np.isnan(fill) else bool(np.all(ws == fill))


@pytest.mark.parametrize("order", ["forward", "reverse"])
@pytest.mark.parametrize("shape", DC.SHAPES, ids=_ids)
def test_tail_backward_against_the_aten_chain(shape, order, monkeypatch):
    c = DC.case(shape)

    def run(fill):
        g, g_b, g_bias_b, g_bias_h, ws = HD.tail_bwd(c["q"], c["y"], c["g_out"], c["w"], DC.ALPHA, True, True, fill)
        g0, g_b0, none_b, none_h, ws0 = HD.tail_bwd(c["q"], c["y"], c["g_out"], c["w"], DC.ALPHA, False, False, fill)
        assert none_b is None and none_h is None and ws_untouched(ws0, fill), "frozen biases must leave ws untouched"
        g1, g_b1, only_b, none_h, _ = HD.tail_bwd(c["q"], c["y"], c["g_out"], c["w"], DC.ALPHA, True, False, fill)
        g2, g_b2, none_b, only_h, _ = HD.tail_bwd(c["q"], c["y"], c["g_out"], c["w"], DC.ALPHA, False, True, fill)
        assert identical((g, g_b) * 3, (g0, g_b0, g1, g_b1, g2, g_b2)), "the sums change what is stored"
        assert identical((g_bias_b, g_bias_h), (only_b, only_h)), "one sum changes the other"
        return g, g_b, g_bias_b, g_bias_h, ws
    g, g_b, g_bias_b, g_bias_h, ws = both_orders_and_fills(run, order, monkeypatch)
    al, one = np.float32(DC.ALPHA), np.float32(1)
    want_g = (((c["g_out"] * al).astype(np.float32) * (one - c["y"])).astype(np.float32) * c["y"]).astype(np.float32)
    assert np.array_equal(g.view(np.uint32), want_g.view(np.uint32)), "g is not disp_head_bwd_kernel's expression"
    assert not np.isnan(ws).any()
    worst = {}
    for name, got in (("g_b", g_b), ("g_bias_b", g_bias_b), ("g_bias_head", g_bias_h)):
        worst[name] = DC.ratio(got, c["ref32"][name], c["ref64"][name], c["S"][name])
        assert worst[name] <= 1.0, (shape, name, worst[name])
    # the sums are the fp64 sums of what was stored, rounded once
    mag = np.abs(g_b.astype(np.float64)).sum(axis=(0, 2, 3))
    assert np.all(np.abs(g_bias_b - g_b.astype(np.float64).sum(axis=(0, 2, 3))) <= 2.0 ** -23 * mag)
    assert abs(float(g_bias_h[0]) - g.astype(np.float64).sum()) <= 2.0 ** -23 * np.abs(g.astype(np.float64)).sum()
    report(f"tail backward on the simulator {shape} {order}: worst entry of g_b at {worst['g_b']:.3f}, of its bias sum "
           f"at {worst['g_bias_b']:.3f}, the head's bias at {worst['g_bias_head']:.3f} of the bound")


@pytest.mark.parametrize("order", ["forward", "reverse"])
@pytest.mark.parametrize("shape", DC.SHAPES, ids=_ids)
def test_exact_inputs_give_the_fp64_result(shape, order, monkeypatch):
    q, g_in, w = DC.exact_case(shape)

    def run(fill):
        return HD.tail_bwd(q, None, g_in, w, DC.ALPHA, True, True, fill)
    g, g_b, g_bias_b, g_bias_h, _ = both_orders_and_fills(run, order, monkeypatch)
    want_b, want_bias_b, want_bias_h = DC.tail_ref64(q, g_in, w)
    assert np.array_equal(g, g_in), "null-y mode must hand g_out through"
    assert g_b.dtype == np.float32 and np.array_equal(g_b.astype(np.float64), want_b), DC.first_difference(g_b, want_b)
    assert np.array_equal(g_bias_b.astype(np.float64), want_bias_b)
    assert np.array_equal(g_bias_h.astype(np.float64), want_bias_h)


@pytest.mark.parametrize("shape", DC.SHAPES, ids=_ids)
def test_impulses_return_the_flipped_window_with_its_folds(shape):
    B, H, W = shape
    for pos in DC.impulse_positions(H, W):
        q, g_in, w = DC.impulse_case(shape, pos)
        _, g_b, g_bias_b, g_bias_h, _ = HD.tail_bwd(q, None, g_in, w, DC.ALPHA)
        want_b, want_bias_b, _ = DC.tail_ref64(q, g_in, w)
        assert np.array_equal(g_b.astype(np.float64), want_b), (pos, DC.first_difference(g_b, want_b))
        assert np.array_equal(g_bias_b.astype(np.float64), want_bias_b) and float(g_bias_h[0]) == 1.0, pos
        # every weight is returned once per padded position it reaches: 9 positions, all inside the padded grid
        assert np.array_equal(want_bias_b, w.reshape(DC.C, 9).sum(axis=1).astype(np.float64)), pos


def test_the_shapes_cover_corners_partial_tiles_and_several_tiles():
    tiles = lambda H, W: (-(-H // 8), -(-W // 64))  # noqa: E731
    assert (1, 2, 2) in DC.SHAPES
    assert {tiles(H, W) for _, H, W in DC.SHAPES} >= {(1, 1), (3, 2), (2, 3)}
    assert any(H % 8 and W % 64 and B > 1 for B, H, W in DC.SHAPES)
    n = HD.ws_bytes(2, 16, 17, 67)
    assert n == 8 * 17 * 2 * 3 * 2 and HD.ws_bytes(12, 16, 256, 832) == 8 * 17 * 12 * 32 * 13


def _ptr(a):
    return ctypes.c_void_p(a.ctypes.data)


def _nan(*shape, dtype=np.float32):
    return np.full(shape, np.nan, dtype)


def test_rejected_arguments_return_minus_one_and_write_nothing():
    B, C, H, W = 2, 16, 4, 5
    q, y = np.ones((B, C, H + 2, W + 2), np.float32), np.full((B, 1, H, W), 0.5, np.float32)
    g_out, w = np.ones((B, 1, H, W), np.float32), np.ones((1, C, 3, 3), np.float32)
    n = HD.ws_bytes(B, C, H, W)
    g, g_b, ws, g_bias_b, g_bias_h = _nan(B, 1, H, W), _nan(B, C, H, W), _nan(n // 8 + 1, dtype=np.float64), _nan(C), _nan(1)
    fn = HD.lib()._fn["scsfm_dgrad_head_tail_bwd_f32"]
    good = [B, C, H, W, 10.0, _ptr(q), _ptr(y), _ptr(g_out), _ptr(w), _ptr(g), _ptr(g_b), _ptr(ws), n, _ptr(g_bias_b),
            _ptr(g_bias_h), None]
    table = [{0: 0}, {0: -1}, {1: 8}, {1: 17}, {1: 32}, {2: 1}, {2: 0}, {3: 1}, {3: -2}, {5: None}, {7: None}, {8: None},
             {9: None}, {10: None}, {11: None}, {12: n - 1}, {12: 0}, {11: ctypes.c_void_p(ws.ctypes.data + 4)},
             {0: 1 << 14, 2: 1 << 7, 3: 1 << 6}]  # 2^14 x 16 x 130 x 66 padded entries: past 2^31
    for bad in table:
        args = list(good)
        for k, v in bad.items():
            args[k] = v
        assert fn(*args) == -1, bad
        assert all(np.isnan(o).all() for o in (g, g_b, ws, g_bias_b, g_bias_h)), bad
    # without sums the workspace is not needed
    args = list(good)
    args[11], args[12], args[13], args[14] = None, 0, None, None
    assert fn(*args) == 0 and not np.isnan(g).any() and not np.isnan(g_b).any()
    assert HD.lib()._fn["scsfm_dgrad_source_id"](None, 64) == -1
    assert HD.ws_bytes(0, 16, 4, 4) == 0 and HD.ws_bytes(1, 16, 1, 4) == 0 and HD.ws_bytes(1, 8, 4, 4) == 0
    covers = HD.lib()._fn["scsfm_dgrad_head_tail_covers"]
    assert [covers(c) for c in (1, 8, 16, 17, 32)] == [0, 0, 1, 0, 0]
