"""The decoder-bias kernels (csrc_decb/scsfm_decoder_bias.hip) on the host simulator (tests/_hostsim_decb.py).

Forward: bit-identical to a float32 numpy restatement (every step one fp32 numpy operation; expm1f and expf are the C
library's, the functions the simulated kernel calls -- numpy's own float32 exp is a different implementation).
Backward: g_x, g_a and g_skip bit-identical to the restatements of tests/_decoder_ref.py on the same `out`, the head's
to ((g * alpha) * (1 - y)) * y in float32; g_bias within 2^-23 * sum|terms| of numpy's fp64 sum of the stored gradient
(the fixed-order fp64 sum rounded once to fp32 is within half an ulp of it).  Every case runs twice (same bits), in both
thread orders, with two prefills of the outputs and the workspace (NaN bytes and a finite value), between NaN guard
bands, with randn inputs and with a 40 % special-value fill.  Then the whole DepthDecoder.forward_fused_bias over the
simulator against forward_reference in fp32 and fp64."""
import copy
import ctypes
import ctypes.util
import itertools

import numpy as np
import pytest
import torch

import _decoder_ref as R
import _hostsim_decb as HB
import _hostsim_nets as HS
from _util import report

OTHER_FILL = 12345.0
_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
for _f in (_libm.expm1f, _libm.expf):
    _f.restype, _f.argtypes = ctypes.c_float, [ctypes.c_float]


def _map(fn, v):
    return np.array([fn(float(t)) for t in v.ravel()], np.float32).reshape(v.shape)


def same(a, b):
    """the same bits, NaN matching NaN"""
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(R.bits(a)[~na], R.bits(b)[~nb])


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


def elu32(v):
    with np.errstate(all="ignore"):
        return np.where(v > 0, v, _map(_libm.expm1f, v)).astype(np.float32)


def add_bias(x, bias):
    with np.errstate(all="ignore"):
        return (x + bias.reshape(1, -1, 1, 1)).astype(np.float32)


def pad32(v):
    return np.pad(v, ((0, 0), (0, 0), (1, 1), (1, 1)), mode="reflect")


def check_bias_grad(name, g_bias, stored, kind):
    """|g_bias - sum64| <= 2^-23 * sum|terms| per channel; a non-finite sum (special fill) must come out as it is"""
    s64 = stored.astype(np.float64)
    with np.errstate(all="ignore"):
        want, mag = s64.sum(axis=(0, 2, 3)), np.abs(s64).sum(axis=(0, 2, 3))
        want32 = want.astype(np.float32)
    assert g_bias.shape == want.shape and g_bias.dtype == np.float32, name
    fin = np.isfinite(mag) & np.isfinite(want32)
    assert kind == "special" or fin.all(), name
    assert same(g_bias[~fin], want32[~fin]), f"{name}: {g_bias[~fin]} for {want32[~fin]}"
    d = np.abs(g_bias[fin].astype(np.float64) - want[fin])
    assert np.all(d <= 2.0 ** -23 * mag[fin]), f"{name}: {d} against {2.0 ** -23 * mag[fin]}"


def ws_untouched(ws, fill):
    return np.isnan(ws).all() if np.isnan(fill) else bool(np.all(ws == fill))


# -------------------------------------------------------------------------------------------------- elu_pad

ELU_W = (2, 3, 254, 255, 256, 257, 258, 513)
ELU_BCH = list(itertools.product((1, 2), (1, 3, 5), (2, 3, 5)))


@pytest.mark.parametrize("order", ["forward", "reverse"])
@pytest.mark.parametrize("kind", ["randn", "special"])
@pytest.mark.parametrize("W", ELU_W)
def test_bias_elu_pad(W, kind, order, monkeypatch):
    for B, C, H in ELU_BCH:
        shape = (B, C, H, W)
        rng = np.random.default_rng(sum(shape) + 7 * C + (kind == "special"))
        x, bias = R.fill(shape, kind, rng), R.fill((C,), kind, rng)
        gp = R.fill((B, C, H + 2, W + 2), kind, rng)

        def run(fill):
            out = HB.bias_elu_pad_fwd(x, bias, fill)
            g_x, g_bias, ws = HB.bias_elu_pad_bwd(gp, out, True, fill)
            g_x0, none, ws0 = HB.bias_elu_pad_bwd(gp, out, False, fill)
            assert none is None and ws_untouched(ws0, fill), "a NULL g_bias must leave ws untouched"
            return out, g_x, g_bias, ws, g_x0
        out, g_x, g_bias, ws, g_x0 = both_orders_and_fills(run, order, monkeypatch)
        name = f"bias_elu_pad {shape} {kind}"
        assert same(out, pad32(elu32(add_bias(x, bias)))), name
        exact = R.pad_bwd_32(gp, out, True)
        assert same(g_x, exact) and same(g_x0, exact), name
        assert same(g_x, HS.pad_bwd(gp, out, True)), name  # (what scsfm_nets_pad_bwd_f32 stores)
        assert not np.isnan(ws).any() or kind == "special", name
        check_bias_grad(name, g_bias, g_x, kind)


# ----------------------------------------------------------------------------------------------- up_cat_pad

UP_W = (2, 3, 127, 128, 129)
UP_BCH = list(itertools.product((1, 2), ((1, 0), (3, 2), (5, 0)), (1, 2, 3)))


@pytest.mark.parametrize("order", ["forward", "reverse"])
@pytest.mark.parametrize("kind", ["randn", "special"])
@pytest.mark.parametrize("W", UP_W)
def test_bias_up_cat_pad(W, kind, order, monkeypatch):
    for B, (Ca, Cs), H in UP_BCH:
        shape = (B, Ca, Cs, H, W)
        rng = np.random.default_rng(sum(shape) + 7 * Ca + (kind == "special"))
        a, bias = R.fill((B, Ca, H, W), kind, rng), R.fill((Ca,), kind, rng)
        skip = R.fill((B, Cs, 2 * H, 2 * W), kind, rng)
        gp = R.fill((B, Ca + Cs, 2 * H + 2, 2 * W + 2), kind, rng)

        def run(fill):
            out = HB.bias_up_cat_pad_fwd(a, bias, skip, fill)
            g_a, g_skip, g_bias, ws = HB.bias_up_cat_pad_bwd(gp, out, Ca, True, fill)
            g_a0, g_skip0, none, ws0 = HB.bias_up_cat_pad_bwd(gp, out, Ca, False, fill)
            assert none is None and ws_untouched(ws0, fill), "a NULL g_bias must leave ws untouched"
            return out, g_a, g_skip, g_bias, ws, g_a0, g_skip0
        out, g_a, g_skip, g_bias, ws, g_a0, g_skip0 = both_orders_and_fills(run, order, monkeypatch)
        name = f"bias_up_cat_pad {shape} {kind}"
        up = elu32(add_bias(a, bias)).repeat(2, 2).repeat(2, 3)
        assert same(out, pad32(np.concatenate([up, skip], 1))), name
        exact_a, exact_s = R.up_cat_pad_bwd_32(gp, out, Ca)
        assert same(g_a, exact_a) and same(g_a0, exact_a), name
        assert (g_skip is None) == (Cs == 0) == (g_skip0 is None), name
        if Cs:
            assert same(g_skip, exact_s) and same(g_skip0, exact_s), name
        nets_a, nets_s = HS.up_cat_pad_bwd(gp, out, Ca)
        assert same(g_a, nets_a) and (Cs == 0 or same(g_skip, nets_s)), name
        check_bias_grad(name, g_bias, g_a, kind)  # (the skip half contributes nothing)


# ----------------------------------------------------------------------------------------------------- head

HEAD_SHAPES = [(B, 1, H, W) for B in (1, 2) for H, W in ((2, 2), (5, 51), (1, 255), (16, 16), (1, 257))] + \
    [(2, 3, 1, 257)]


@pytest.mark.parametrize("order", ["forward", "reverse"])
@pytest.mark.parametrize("kind", ["randn", "special"])
@pytest.mark.parametrize("shape", HEAD_SHAPES)
def test_disp_head(shape, kind, order, monkeypatch):
    B, C, H, W = shape
    rng = np.random.default_rng(sum(shape) + (kind == "special"))
    x, bias, g_out = R.fill(shape, kind, rng), R.fill((C,), kind, rng), R.fill(shape, kind, rng)
    alpha, beta = 10.0, 0.01

    def run(fill):
        y, out = HB.disp_head_fwd(x, bias, alpha, beta, fill)
        g_x, g_bias, ws = HB.disp_head_bwd(g_out, y, alpha, True, fill)
        g_x0, none, ws0 = HB.disp_head_bwd(g_out, y, alpha, False, fill)
        assert none is None and ws_untouched(ws0, fill), "a NULL g_bias must leave ws untouched"
        return y, out, g_x, g_bias, ws, g_x0
    y, out, g_x, g_bias, ws, g_x0 = both_orders_and_fills(run, order, monkeypatch)
    name = f"disp_head {shape} {kind}"
    one, al, be = np.float32(1), np.float32(alpha), np.float32(beta)
    with np.errstate(all="ignore"):
        want_y = (one / (one + _map(_libm.expf, -add_bias(x, bias)))).astype(np.float32)
        want_out = ((al * want_y).astype(np.float32) + be).astype(np.float32)
        want_g = ((((g_out * al).astype(np.float32)) * (one - y)).astype(np.float32) * y).astype(np.float32)
    assert same(y, want_y) and same(out, want_out), name
    assert same(g_x, want_g) and same(g_x0, want_g), name
    check_bias_grad(name, g_bias, g_x, kind)


def test_the_shapes_cover_partial_workgroups_and_several_chunks():
    chunks = lambda n: -(-n // 256)  # noqa: E731
    assert any(B * C * H * chunks(W) % 4 for B, C, H in ELU_BCH for W in ELU_W)
    assert {chunks(W) for W in ELU_W} == {1, 2, 3} and {chunks(W + 2) for W in ELU_W} == {1, 2, 3}
    assert {chunks(2 * W + 2) for W in UP_W} == {1, 2} and {chunks(2 * W) for W in UP_W} == {1, 2}
    assert {chunks(H * W) for _, _, H, W in HEAD_SHAPES} == {1, 2}
    # the per-channel sum walks more partials than one pass of its 256 threads only at sizes the GPU tests run; here it
    # crosses planes (B > 1) and rows (H > 1), and a channel's partials are not contiguous (C > 1)
    assert any(B > 1 and C > 1 and H > 1 for B, C, H in ELU_BCH)


def test_the_bias_sum_adds_more_partials_than_threads():
    """B * H * chunks > 256 partials per channel: a thread of the finalising workgroup adds several, 256 apart"""
    B, C, H, W = 3, 2, 90, 2
    rng = np.random.default_rng(5)
    gp = R.fill((B, C, H + 2, W + 2), "randn", rng)
    out = HB.bias_elu_pad_fwd(R.fill((B, C, H, W), "randn", rng), R.fill((C,), "randn", rng))
    g_x, g_bias, ws = HB.bias_elu_pad_bwd(gp, out)
    assert ws.size == B * C * H and same(g_x, R.pad_bwd_32(gp, out, True))
    assert np.array_equal(ws.reshape(B, C, H), g_x.astype(np.float64).sum(axis=3))  # (two terms: exact in fp64)
    check_bias_grad("many partials", g_bias, g_x, "randn")


# ------------------------------------------------------------------------------------------------ rejections

def _ptr(a):
    return ctypes.c_void_p(a.ctypes.data)


def _nan(*shape, dtype=np.float32):
    return np.full(shape, np.nan, dtype)


def _reject(name, good, table, outs):
    fn = HB.lib()._fn[name]
    for bad in table:
        args = list(good)
        for k, v in bad.items():
            args[k] = v
        assert fn(*args) == -1, (name, bad)
        assert all(np.isnan(o).all() for o in outs), (name, bad)


def test_rejected_arguments_return_minus_one_and_write_nothing():
    B, C, Cs, H, W = 2, 3, 2, 4, 5
    big = {0: 1 << 14, 1: 1 << 13, 2: 2, 3: 2}  # 2^27 planes of 4 x 4 padded entries: 2^31 elements
    dims = [(0, 0), (0, -1), (1, 0), (1, -2), (2, 1), (2, 0), (2, -1), (3, 1), (3, 0), (3, -3)]
    x, bias, out = np.ones((B, C, H, W), np.float32), np.ones(C, np.float32), _nan(B, C, H + 2, W + 2)
    _reject("scsfm_decb_bias_elu_pad_fwd_f32", [B, C, H, W, _ptr(x), _ptr(bias), _ptr(out), None],
            [{k: v} for k, v in dims + [(4, None), (5, None), (6, None)]] + [big], [out])
    gp, res = np.ones(out.shape, np.float32), np.ones(out.shape, np.float32)
    g_x, ws, g_b = _nan(B, C, H, W), _nan(B * C * H, dtype=np.float64), _nan(C)
    _reject("scsfm_decb_bias_elu_pad_bwd_f32", [B, C, H, W, _ptr(gp), _ptr(res), _ptr(g_x), _ptr(ws), _ptr(g_b), None],
            [{k: v} for k, v in dims + [(4, None), (5, None), (6, None), (7, None)]] + [big], [g_x, ws, g_b])

    big = {0: 1 << 14, 1: 1 << 13, 2: 0, 3: 1, 4: 1}  # 2^27 planes of 4 x 4
    dims = [(0, 0), (0, -1), (1, 0), (1, -1), (2, -1), (3, 0), (3, -1), (4, 0), (4, -2)]
    a, skip = np.ones((B, C, H, W), np.float32), np.ones((B, Cs, 2 * H, 2 * W), np.float32)
    out = _nan(B, C + Cs, 2 * H + 2, 2 * W + 2)
    _reject("scsfm_decb_bias_up_cat_pad_fwd_f32", [B, C, Cs, H, W, _ptr(a), _ptr(bias), _ptr(skip), _ptr(out), None],
            [{k: v} for k, v in dims + [(5, None), (6, None), (7, None), (8, None)]] + [big], [out])
    gp, res = np.ones(out.shape, np.float32), np.ones(out.shape, np.float32)
    g_a, g_skip = _nan(*a.shape), _nan(*skip.shape)
    _reject("scsfm_decb_bias_up_cat_pad_bwd_f32",
            [B, C, Cs, H, W, _ptr(gp), _ptr(res), _ptr(g_a), _ptr(g_skip), _ptr(ws), _ptr(g_b), None],
            [{k: v} for k, v in dims + [(5, None), (6, None), (7, None), (8, None), (9, None)]] + [big],
            [g_a, g_skip, ws, g_b])

    big = {0: 1 << 14, 1: 1 << 13, 2: 4, 3: 4}
    dims = [(0, 0), (0, -1), (1, 0), (1, -2), (2, 0), (2, -1), (3, 0), (3, -3)]
    y, out = _nan(B, C, H, W), _nan(B, C, H, W)
    _reject("scsfm_decb_disp_head_fwd_f32", [B, C, H, W, _ptr(x), _ptr(bias), 10.0, 0.01, _ptr(y), _ptr(out), None],
            [{k: v} for k, v in dims + [(4, None), (5, None), (8, None), (9, None)]] + [big], [y, out])
    g_out, yy = np.ones((B, C, H, W), np.float32), np.full((B, C, H, W), 0.5, np.float32)
    _reject("scsfm_decb_disp_head_bwd_f32", [B, C, H, W, 10.0, _ptr(g_out), _ptr(yy), _ptr(g_x), _ptr(ws), _ptr(g_b),
                                            None],
            [{k: v} for k, v in dims + [(5, None), (6, None), (7, None), (8, None)]] + [big], [g_x, ws, g_b])
    assert HB.lib()._fn["scsfm_decb_source_id"](None, 64) == -1
    assert HB.ws_bytes(0, 1, 1, 1) == 0 and HB.ws_bytes(2, 3, 4, 257) == 8 * 2 * 3 * 4 * 2


# ------------------------------------------------------------------ the whole decoder over the simulator, on the CPU

NUM_CH_ENC = [4, 4, 8, 8, 16]
VARIANTS = [(size, sk, sc, al) for size in ((2, 3), (2, 17)) for sk in (True, False) for sc in (range(4), [1, 2])
            for al in (False, True)]


def _features(h, w, dtype=torch.float32):
    g = torch.Generator().manual_seed(100 * h + w)
    return [torch.randn(2, c, h << (4 - k), w << (4 - k), generator=g).to(dtype) for k, c in enumerate(NUM_CH_ENC)]


def _decoder_run(dec, feats, weights, num_scales, fused):
    feats = [f.clone().requires_grad_() for f in feats]
    outs = dec.forward_fused_bias(feats) if fused else dec.forward_reference(feats)
    loss = sum((o * w.to(o.dtype)).sum() for o, w in zip(outs[:num_scales], weights))
    grads = torch.autograd.grad(loss, feats + list(dec.parameters()), allow_unused=True)
    return [o.detach() for o in outs] + list(grads)


@pytest.mark.parametrize("size,use_skips,scales,all_scales", VARIANTS, ids=[
    f"{h}x{w}-{'skips' if sk else 'no_skips'}-heads{''.join(map(str, sc))}-{'all_scales' if al else 'one_scale'}"
    for (h, w), sk, sc, al in VARIANTS])
def test_the_whole_decoder_with_folded_biases_on_the_simulator(size, use_skips, scales, all_scales, monkeypatch):
    """forward_fused_bias (fp32, the glue on the simulator) is as close to the fp64 reference chain as the fp32
    reference chain is, for every output, feature gradient and parameter gradient (the bound and the positive loss
    weights of tests/test_decoder_hostsim.py: test_the_whole_decoder_on_the_simulator, whose docstring explains both):
    max|new32 - ref64| <= 2 max|ref32 - ref64| + 1e-7 max|ref64|."""
    from models.DispResNet import DepthDecoder
    from scsfm_hip import decoder as D, decoder_bias as DB
    monkeypatch.setattr(D, "pad", HS.pad)
    for name in ("elu_pad", "up_cat_pad", "disp_head"):
        monkeypatch.setattr(DB, name, getattr(HB, name))
    torch.manual_seed(7)
    dec = DepthDecoder(NUM_CH_ENC, scales=scales, use_skips=use_skips).float()
    dec64 = copy.deepcopy(dec).double()
    feats = _features(*size)
    assert not dec.fused_path_applies(feats)
    n_out = len(list(scales))
    g = torch.Generator().manual_seed(11)
    weights = [torch.rand(2, 1, (size[0] << 5) >> s, (size[1] << 5) >> s, generator=g) + 0.5 for s in list(scales)]
    num_scales = n_out if all_scales else 1
    new = _decoder_run(dec, feats, weights, num_scales, True)
    ref32 = _decoder_run(dec, feats, weights, num_scales, False)
    ref64 = _decoder_run(dec64, [f.double() for f in feats], weights, num_scales, False)
    assert len(new) == len(ref32) == len(ref64) == n_out + 5 + len(list(dec.parameters()))
    worst, used = 0.0, 0
    for k, (a, b, c) in enumerate(zip(new, ref32, ref64)):
        assert (a is None) == (b is None) == (c is None), k
        if a is None:
            continue
        used += 1
        assert a.shape == c.shape and a.dtype == torch.float32, k
        err, yard, scale = float((a.double() - c).abs().max()), float((b.double() - c).abs().max()), float(c.abs().max())
        assert err <= 2 * yard + 1e-7 * scale, (k, tuple(a.shape), err, yard, scale)
        worst = max(worst, err / (yard + 0.5e-7 * scale + 1e-300))
    assert used > n_out + 1
    report(f"decoder with folded biases on the simulator {size} skips={use_skips} heads={list(scales)} "
           f"num_scales={num_scales}: at {worst:.2f} x the fp32 reference chain's own error ({used} tensors)")
