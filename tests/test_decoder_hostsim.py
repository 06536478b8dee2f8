"""The depth decoder's fused glue (csrc_nets/scsfm_decoder.hip) on the host simulator (tests/_hostsim_nets.py) against
the two numpy references of tests/_decoder_ref.py: the forward against the padded source (copies, bit for bit) and the
float64 yardstick (ELU results, 1 ulp), the backward bit for bit against the documented order restated in float32 and,
on random inputs, within 8 u * sum|terms| of the float64 transpose.  Every case runs in both thread orders (a result that
changes is a race) and with two different output prefills (an entry that differs was never written).  Then the whole
DepthDecoder.forward_fused over the simulator against forward_reference in fp32 and fp64."""
import copy
import ctypes
import itertools

import numpy as np
import pytest
import torch

import _decoder_ref as R
import _hostsim_nets as HS
from _util import report

PAD_SHAPES = R.ODD_PAD + R.CHUNK_PAD + [(2, 8, 16, 52)]
UP_SHAPES = R.ODD_UP + R.CHUNK_UP + [(2, 16, 8, 16, 52)]
OTHER_FILL = 12345.0  # the second, finite prefill
NEG_ZERO = np.float32(-0.0).view(np.int32)


def same(a, b):
    """the same bits, NaN matching NaN"""
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(R.bits(a)[~na], R.bits(b)[~nb])


def identical(xs, ys):
    assert len(xs) == len(ys) and all((x is None) == (y is None) and (x is None or x.shape == y.shape)
                                      for x, y in zip(xs, ys))
    return all((x is None and y is None) or np.array_equal(R.bits(x), R.bits(y)) for x, y in zip(xs, ys))


def check_forward(name, out, src, copied, ref64):
    """src: the padded (upsampled, concatenated) fp32 source; copied: where the output is a copy of it"""
    assert out.shape == src.shape == ref64.shape, name
    assert np.array_equal(R.bits(out)[copied], R.bits(src)[copied]), f"{name}: a copied entry differs"
    rest, nan = ~copied, np.isnan(ref64)
    assert np.array_equal(np.isnan(out)[rest], nan[rest]), f"{name}: NaN positions"
    zero = rest & (R.bits(src) == NEG_ZERO)
    assert np.all(R.bits(out)[zero] == NEG_ZERO), f"{name}: -0 did not stay -0"
    fin = rest & ~nan
    ulp = R.ulp_distance(out[fin], ref64[fin].astype(np.float32))
    assert ulp.size == 0 or int(ulp.max()) <= 1, f"{name}: ELU {int(ulp.max())} ulp from the fp64 result"


def check_backward(name, got, exact, ref64, mag, kind):
    assert same(got, exact), f"{name}: not the documented order's bits"
    if kind == "randn":
        d = np.abs(got.astype(np.float64) - ref64)
        bound = 8 * R.U * mag + 1e-45
        assert np.all(d <= bound), f"{name}: {float((d / bound).max()):.2f} x the bound"


def both_orders_and_fills(run, order, monkeypatch):
    """run(fill) -> tuple of arrays; the results of the NaN-prefilled run in the asked thread order, after checking that
    the other order and the other prefill give the same bits"""
    monkeypatch.delenv("HOSTSIM_ORDER", raising=False)
    first = run(np.nan)
    if order == "reverse":
        monkeypatch.setenv("HOSTSIM_ORDER", "reverse")
        got = run(np.nan)
        assert identical(first, got), "the thread order changes the result"
    else:
        got = first
    assert identical(got, run(OTHER_FILL)), "an output entry keeps its prefill"
    return got


@pytest.mark.parametrize("order", ["forward", "reverse"])
@pytest.mark.parametrize("kind", ["randn", "special"])
@pytest.mark.parametrize("elu", [False, True])
@pytest.mark.parametrize("shape", PAD_SHAPES)
def test_pad(shape, elu, kind, order, monkeypatch):
    B, C, H, W = shape
    rng = np.random.default_rng(sum(shape) + 2 * elu + (kind == "special"))
    x, gp = R.fill(shape, kind, rng), R.fill((B, C, H + 2, W + 2), kind, rng)

    def run(fill):
        out = HS.pad_fwd(x, elu, fill)
        return out, HS.pad_bwd(gp, out, elu, fill)
    out, g_x = both_orders_and_fills(run, order, monkeypatch)
    src = np.pad(x, ((0, 0), (0, 0), (1, 1), (1, 1)), mode="reflect")
    check_forward(f"pad {shape}", out, src, (src > 0) if elu else np.ones(src.shape, bool), R.pad_fwd_64(x, elu))
    ref, mag = R.pad_bwd_64(gp, out, elu)
    check_backward(f"pad {shape} g_x", g_x, R.pad_bwd_32(gp, out, elu), ref, mag, kind)


@pytest.mark.parametrize("order", ["forward", "reverse"])
@pytest.mark.parametrize("kind", ["randn", "special"])
@pytest.mark.parametrize("shape", UP_SHAPES)
def test_up_cat_pad(shape, kind, order, monkeypatch):
    B, Ca, Cs, H, W = shape
    rng = np.random.default_rng(sum(shape) + (kind == "special"))
    a, skip = R.fill((B, Ca, H, W), kind, rng), R.fill((B, Cs, 2 * H, 2 * W), kind, rng)
    gp = R.fill((B, Ca + Cs, 2 * H + 2, 2 * W + 2), kind, rng)

    def run(fill):
        out = HS.up_cat_pad_fwd(a, skip, fill)
        return (out,) + HS.up_cat_pad_bwd(gp, out, Ca, fill)
    out, g_a, g_skip = both_orders_and_fills(run, order, monkeypatch)
    src = np.pad(np.concatenate([a.repeat(2, 2).repeat(2, 3), skip], 1), ((0, 0), (0, 0), (1, 1), (1, 1)), mode="reflect")
    copied = src > 0
    copied[:, Ca:] = True
    check_forward(f"up_cat_pad {shape}", out, src, copied, R.up_cat_pad_fwd_64(a, skip))
    ref_a, ref_s, mag_a, mag_s = R.up_cat_pad_bwd_64(gp, out, Ca)
    exact_a, exact_s = R.up_cat_pad_bwd_32(gp, out, Ca)
    check_backward(f"up_cat_pad {shape} g_a", g_a, exact_a, ref_a, mag_a, kind)
    assert (g_skip is None) == (Cs == 0)
    if Cs:
        check_backward(f"up_cat_pad {shape} g_skip", g_skip, exact_s, ref_s, mag_s, kind)


def test_the_shapes_cover_partial_workgroups_and_batched_skips():
    """a workgroup holds four segments: each launch has a shape whose last workgroup is partly empty"""
    chunks = lambda n: -(-n // 256)  # noqa: E731
    assert any(B * C * (H + 2) * chunks(W + 2) % 4 for B, C, H, W in PAD_SHAPES)
    assert any(B * C * H * chunks(W) % 4 for B, C, H, W in PAD_SHAPES)
    assert any(B * (Ca + Cs) * (2 * H + 2) * chunks(2 * W + 2) % 4 for B, Ca, Cs, H, W in UP_SHAPES)
    assert any((B * Ca * H * chunks(W) + B * Cs * 2 * H * chunks(2 * W)) % 4 for B, Ca, Cs, H, W in UP_SHAPES)
    assert any(B > 1 and Cs > 0 for B, Ca, Cs, H, W in UP_SHAPES)
    # the skip rows need another number of chunks than the a rows
    assert any(Cs > 0 and chunks(W) != chunks(2 * W) for B, Ca, Cs, H, W in UP_SHAPES)


# ------------------------------------------------------------------------------------ explicit, readable cases

def test_an_interior_gradient_of_minus_zero_comes_back_as_plus_zero():
    """an entry with one term is 0 + g (ATen zero-fills and adds): -0 becomes +0, in every op of the backward"""
    gp = np.full((1, 1, 7, 7), -0.0, np.float32)
    assert np.all(R.bits(gp) == NEG_ZERO)
    x = np.ones((1, 1, 5, 5), np.float32)
    for elu in (False, True):
        g_x = HS.pad_bwd(gp, HS.pad_fwd(x, elu), elu)
        assert np.all(R.bits(g_x) == 0), elu  # (2, 2) has one term; the others add further -0 to +0
    gp = np.full((1, 2, 6, 6), -0.0, np.float32)
    out = HS.up_cat_pad_fwd(np.ones((1, 1, 2, 2), np.float32), np.ones((1, 1, 4, 4), np.float32))
    g_a, g_skip = HS.up_cat_pad_bwd(gp, out, 1)
    assert np.all(R.bits(g_a) == 0) and np.all(R.bits(g_skip) == 0)


def _sum32(terms):
    acc = np.float32(0)
    for t in terms:
        acc = np.float32(acc + np.float32(t))
    return acc


def test_a_corner_adds_its_four_terms_in_the_documented_order():
    """Corner (cy, cx) of a 6 x 8 plane, cy in (1, H-2), cx in (1, W-2): its terms are g[cy+1][cx+1], the reflected
    column of that row, then the reflected row at cx+1 and at the reflected column.  With (-1, -u, 1 + 2u, 1.5u),
    u = 2^-24: -1 - u rounds to -1, + (1 + 2u) = 2u, + 1.5u = 3.5u.  No other order gives these bits (but for swapping
    the first two, which 0 + a + b cannot tell apart)."""
    u = 2.0 ** -24
    terms = (-1.0, -u, 1 + 2 * u, 1.5 * u)
    want = _sum32(terms)
    assert float(want) == 3.5 * u
    orders = [p for p in itertools.permutations(range(4)) if _sum32([terms[i] for i in p]).view(np.int32) ==
              want.view(np.int32)]
    assert orders == [(0, 1, 2, 3), (1, 0, 2, 3)]
    H, W = 6, 8
    for cy, ry in ((1, 0), (H - 2, H + 1)):
        for cx, rx in ((1, 0), (W - 2, W + 1)):
            gp = np.zeros((1, 1, H + 2, W + 2), np.float32)
            gp[0, 0, cy + 1, cx + 1], gp[0, 0, cy + 1, rx], gp[0, 0, ry, cx + 1], gp[0, 0, ry, rx] = terms
            for got in (HS.pad_bwd(gp, None, False),
                        HS.pad_bwd(gp, HS.pad_fwd(np.ones((1, 1, H, W), np.float32), True), True),
                        HS.up_cat_pad_bwd(np.concatenate([gp, gp], 1), np.ones((1, 2, H + 2, W + 2), np.float32), 1)[1]):
                assert got[0, 0, cy, cx].view(np.int32) == want.view(np.int32), (cy, cx, float(got[0, 0, cy, cx]) / u)
                assert same(got, R.fold_32(gp))


def test_upsample_children_are_summed_row_major_from_zero():
    """children (1, u / -1, u): ((1 + u) - 1) + u = u row-major, 2u column-major (the GPU test's case, on the simulator)"""
    u = 2.0 ** -24
    gp = np.zeros((1, 1, 8, 8), np.float32)
    gp[0, 0, 3:5, 3:5] = [[1.0, u], [-1.0, u]]
    out = HS.up_cat_pad_fwd(np.ones((1, 1, 3, 3), np.float32), None)
    g_a, g_skip = HS.up_cat_pad_bwd(gp, out, 1)
    assert g_skip is None and float(g_a[0, 0, 1, 1]) == u and np.count_nonzero(g_a) == 1


def test_saturated_elu_turns_a_negative_gradient_into_minus_zero():
    """r == -1 (x = -104: expm1f saturates): the gradient is g * (r + 1) = g * 0, -0 for g < 0"""
    x = np.full((1, 1, 4, 4), -104.0, np.float32)
    out = HS.pad_fwd(x, True)
    assert np.all(out == -1.0)
    gp = np.zeros((1, 1, 6, 6), np.float32)
    gp[0, 0, 1, 1], gp[0, 0, 4, 4] = -2.0, 3.0  # (0, 0) and (3, 3): one term each
    g_x = HS.pad_bwd(gp, out, True)
    assert g_x[0, 0, 0, 0].view(np.int32) == NEG_ZERO and g_x[0, 0, 3, 3].view(np.int32) == 0
    a = np.full((1, 1, 2, 2), -104.0, np.float32)
    out = HS.up_cat_pad_fwd(a, None)
    gp = np.zeros((1, 1, 6, 6), np.float32)
    gp[0, 0, 1, 1] = -2.0  # a child of a[0][0]
    g_a, _ = HS.up_cat_pad_bwd(gp, out, 1)
    assert g_a[0, 0, 0, 0].view(np.int32) == NEG_ZERO and np.all(R.bits(g_a).ravel()[1:] == 0)


def test_both_zeros_take_the_r_le_0_branch():
    """r == +0 and r == -0 (from x = +0 and x = -0, which the forward keeps) are on the g * (r + 1) side: the gradient is
    g * 1, for a denormal, an infinite and a huge g as well.  (Either branch gives g there: this pins the value.)"""
    x = np.array([0.0, -0.0, 0.0, -0.0] * 4, np.float32).reshape(1, 1, 4, 4)
    out = HS.pad_fwd(x, True)
    assert np.array_equal(R.bits(out[:, :, 1:-1, 1:-1]), R.bits(x))
    g = np.array([R.DENORM, -R.DENORM, np.inf, -3.4e38, 1.5, -R.FLT_MIN, 3.4e38, -np.inf] * 2, np.float32)
    gp = np.zeros((1, 1, 6, 6), np.float32)
    gp[0, 0, 1:-1, 1:-1] = g.reshape(4, 4)
    g_x = HS.pad_bwd(gp, out, True)
    assert np.array_equal(R.bits(g_x), R.bits(R.fold_32(gp)))
    assert g_x[0, 0, 0, 0] == R.DENORM and g_x[0, 0, 0, 3] == np.float32(-3.4e38) and g_x[0, 0, 3, 3] == -np.inf


# ------------------------------------------------------------------------------------------------ rejections

def _ptr(a):
    return ctypes.c_void_p(a.ctypes.data)


def _nan(*shape):
    return np.full(shape, np.nan, np.float32)


def test_rejected_arguments_return_minus_one_and_write_nothing():
    fn = HS.lib()._fn
    B, C, Cs, H, W = 2, 3, 2, 4, 5
    big = {0: 1 << 14, 1: 1 << 13, 2: 2, 3: 2}  # 2^27 planes of 4 x 4 padded entries: 2^31 elements
    dims = [(0, 0), (0, -1), (1, 0), (1, -2), (2, 1), (2, 0), (2, -1), (3, 1), (3, 0), (3, -3)]

    x, out = np.ones((B, C, H, W), np.float32), _nan(B, C, H + 2, W + 2)
    good = [B, C, H, W, 1, _ptr(x), _ptr(out), None]
    table = [{k: v} for k, v in dims + [(5, None), (6, None)]] + [big]
    gp, res, g_x = np.ones(out.shape, np.float32), np.ones(out.shape, np.float32), _nan(B, C, H, W)
    good_b = [B, C, H, W, 1, _ptr(gp), _ptr(res), _ptr(g_x), None]
    table_b = [{k: v} for k, v in dims + [(5, None), (6, None), (7, None)]] + [big]
    for name, good, table, outs in (("scsfm_nets_pad_fwd_f32", good, table, [out]),
                                    ("scsfm_nets_pad_bwd_f32", good_b, table_b, [g_x])):
        for bad in table:
            args = list(good)
            for k, v in bad.items():
                args[k] = v
            assert fn[name](*args) == -1, (name, bad)
            assert all(np.isnan(o).all() for o in outs), (name, bad)
    # without ELU the backward does not read the forward's output: NULL is accepted, and every entry written
    args = list(good_b)
    args[4], args[6] = 0, None
    assert fn["scsfm_nets_pad_bwd_f32"](*args) == 0 and np.array_equal(g_x, R.fold_32(gp))

    big = {0: 1 << 14, 1: 1 << 13, 2: 0, 3: 1, 4: 1}  # 2^27 planes of 4 x 4
    dims = [(0, 0), (0, -1), (1, 0), (1, -1), (2, -1), (3, 0), (3, -1), (4, 0), (4, -2)]
    a, skip = np.ones((B, C, H, W), np.float32), np.ones((B, Cs, 2 * H, 2 * W), np.float32)
    out = _nan(B, C + Cs, 2 * H + 2, 2 * W + 2)
    good = [B, C, Cs, H, W, _ptr(a), _ptr(skip), _ptr(out), None]
    table = [{k: v} for k, v in dims + [(5, None), (6, None), (7, None)]] + [big]
    gp, res = np.ones(out.shape, np.float32), np.ones(out.shape, np.float32)
    g_a, g_skip = _nan(*a.shape), _nan(*skip.shape)
    good_b = [B, C, Cs, H, W, _ptr(gp), _ptr(res), _ptr(g_a), _ptr(g_skip), None]
    table_b = [{k: v} for k, v in dims + [(5, None), (6, None), (7, None), (8, None)]] + [big]
    for name, good, table, outs in (("scsfm_nets_up_cat_pad_fwd_f32", good, table, [out]),
                                    ("scsfm_nets_up_cat_pad_bwd_f32", good_b, table_b, [g_a, g_skip])):
        for bad in table:
            args = list(good)
            for k, v in bad.items():
                args[k] = v
            assert fn[name](*args) == -1, (name, bad)
            assert all(np.isnan(o).all() for o in outs), (name, bad)
    # skip / g_skip may be NULL exactly when there are no skip channels
    out0, g_a0 = _nan(B, C, 2 * H + 2, 2 * W + 2), _nan(*a.shape)
    assert fn["scsfm_nets_up_cat_pad_fwd_f32"](B, C, 0, H, W, _ptr(a), None, _ptr(out0), None) == 0
    gp0 = np.ones(out0.shape, np.float32)
    assert fn["scsfm_nets_up_cat_pad_bwd_f32"](B, C, 0, H, W, _ptr(gp0), _ptr(out0), _ptr(g_a0), None, None) == 0
    assert not np.isnan(out0).any() and not np.isnan(g_a0).any()


# ------------------------------------------------------------------ the whole decoder over the simulator, on the CPU

NUM_CH_ENC = [4, 4, 8, 8, 16]


def _features(h, w, dtype=torch.float32):
    g = torch.Generator().manual_seed(100 * h + w)
    return [torch.randn(2, c, h << (4 - k), w << (4 - k), generator=g).to(dtype) for k, c in enumerate(NUM_CH_ENC)]


def _decoder_run(dec, feats, weights, num_scales, fused):
    feats = [f.clone().requires_grad_() for f in feats]
    outs = dec.forward_fused(feats) if fused else dec.forward_reference(feats)
    loss = sum((o * w.to(o.dtype)).sum() for o, w in zip(outs[:num_scales], weights))
    grads = torch.autograd.grad(loss, feats + list(dec.parameters()), allow_unused=True)
    return [o.detach() for o in outs] + list(grads)


# Every variant at the small size.  At the wide one (level-4 size 3 x 130: its fp64 convolutions on 96 x 4160 outputs and
# ten million simulated threads take some 20 s a case) two variants that between them take each option once; the other
# six run at 2 x 17 instead, whose rows at levels 1 and 0 (136 to 546 elements) still cross the kernels' 256-element chunk.
_ALL = [(sk, sc, al) for sk in (True, False) for sc in (range(4), [1, 2]) for al in (False, True)]
_WIDE = [(True, range(4), True), (False, [1, 2], False)]
VARIANTS = [((2, 3),) + v for v in _ALL] + [((3, 130),) + v for v in _WIDE] + \
    [((2, 17),) + v for v in _ALL if v not in _WIDE]


@pytest.mark.parametrize("size,use_skips,scales,all_scales", VARIANTS, ids=[
    f"{h}x{w}-{'skips' if sk else 'no_skips'}-heads{''.join(map(str, sc))}-{'all_scales' if al else 'one_scale'}"
    for (h, w), sk, sc, al in VARIANTS])
def test_the_whole_decoder_on_the_simulator(size, use_skips, scales, all_scales, monkeypatch):
    """forward_fused (fp32, the glue on the simulator) is as close to the fp64 reference chain as the fp32 reference
    chain is, for every output, feature gradient and parameter gradient:
    max|fused32 - ref64| <= 2 max|ref32 - ref64| + 1e-7 max|ref64|.  The two fp32 runs share the convolutions and differ
    by 1-ulp ELU results and reassociated border sums; a wiring fault is off by the size of the values.
    The loss weights are positive (uniform in [0.5, 1.5)): a head's bias gradient is ONE number, the sum of its weighted
    output gradients over all pixels, and a one-element tensor has no maximum to average over.  With weights of both
    signs that sum cancels to a hundredth of its terms' total, 1-ulp changes of the terms move it by several of its own
    ulps either way, and the fp32 reference chain's error on it is anything between 0.03 and 5 ulp by chance (measured:
    4.0 ulp for the fused chain against 0.03 ulp for the reference on head 1 of one variant) -- no yardstick.  With one
    sign the sum is as large as its terms' total and such changes stay below its ulp, which the 1e-7 term covers."""
    from models.DispResNet import DepthDecoder
    from scsfm_hip import decoder as D
    for name in ("pad", "elu_pad", "up_cat_pad"):
        monkeypatch.setattr(D, name, getattr(HS, name))
    torch.manual_seed(7)
    dec = DepthDecoder(NUM_CH_ENC, scales=scales, use_skips=use_skips).float()
    dec64 = copy.deepcopy(dec).double()
    feats = _features(*size)
    assert not dec.fused_path_applies(feats)
    n_out = len(list(scales))
    g = torch.Generator().manual_seed(11)
    weights = [torch.rand(2, 1, (size[0] << 5) >> s, (size[1] << 5) >> s, generator=g) + 0.5 for s in list(scales)]
    num_scales = n_out if all_scales else 1
    fused = _decoder_run(dec, feats, weights, num_scales, True)
    ref32 = _decoder_run(dec, feats, weights, num_scales, False)
    ref64 = _decoder_run(dec64, [f.double() for f in feats], weights, num_scales, False)
    assert len(fused) == len(ref32) == len(ref64) == n_out + 5 + len(list(dec.parameters()))
    worst, used = 0.0, 0
    for k, (a, b, c) in enumerate(zip(fused, ref32, ref64)):
        assert (a is None) == (b is None) == (c is None), k
        if a is None:
            continue
        used += 1
        assert a.shape == c.shape and a.dtype == torch.float32, k
        err, yard, scale = float((a.double() - c).abs().max()), float((b.double() - c).abs().max()), float(c.abs().max())
        assert err <= 2 * yard + 1e-7 * scale, (k, tuple(a.shape), err, yard, scale)
        worst = max(worst, err / (yard + 0.5e-7 * scale + 1e-300))
    assert used > n_out + 1
    report(f"decoder on the simulator {size} skips={use_skips} heads={list(scales)} num_scales={num_scales}: fused at "
           f"{worst:.2f} x the fp32 reference chain's own error ({used} tensors)")
