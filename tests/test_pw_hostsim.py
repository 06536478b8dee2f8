"""The 1x1-convolution gradient kernels (csrc_pw/scsfm_pointwise.hip) on the host simulator (tests/_hostsim_pw.py),
compiled unchanged; tests/hostsim/wrw_shim.h supplies v_mfma_f32_16x16x4_f32 as the wave-cooperative k-ordered fmaf chain
that the instruction is, in its lane layout.

Every shape of tests/_pw_cases.py runs in both thread orders (same bits) and with two prefills of the outputs and the
workspace, NaN and a finite value (same bits, everything finite), between NaN guard bands, and meets

    per entry  |got - ref64| <= 2 max|ref32 - ref64| + 8 u S

against ATen's CPU results.  The data gradient must besides hold exact zeros at every position the stride skips.  Without a
tolerance: operands from {-1, 0, 1}, for which no sum is ever rounded, must give the fp64 result to the bit."""
import functools

import numpy as np
import pytest
import torch

import _hostsim_pw as HP
import _pw_cases as PC
from _util import report

OTHER_FILL = 12345.0
ALL = PC.SHAPES + PC.MULTI


@functools.lru_cache(maxsize=None)
def case(shape):
    """the operands of a shape (fp32 numpy, read-only) and the references of both gradients, computed once"""
    B, Cin, Cout, H, W, s = shape
    x, dy, w = PC.operands(shape)
    refs_w = PC.wgrad_refs(x, dy, s)
    refs_d = PC.dgrad_refs(dy, w, H, W) if s == 2 else None
    arrays = tuple(t.numpy() for t in (x, dy, w.reshape(Cout, Cin)))
    for a in arrays:
        a.setflags(write=False)
    return arrays, refs_w, refs_d


def identical(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _orders(monkeypatch, call):
    """call() in forward order, in reverse order and over the other prefill: the same bits; -> the first result"""
    monkeypatch.delenv("HOSTSIM_ORDER", raising=False)
    first = call(np.nan)
    monkeypatch.setenv("HOSTSIM_ORDER", "reverse")
    rev = call(np.nan)
    monkeypatch.delenv("HOSTSIM_ORDER")
    other = call(OTHER_FILL)
    for a, b, c in zip(first, rev, other):
        assert identical(a, b), "the thread order changes the result"
        assert identical(a, c), "an output or workspace entry keeps its prefill"
        assert np.isfinite(a).all(), "an output or workspace entry was left unwritten (NaN prefill)"
    return first


@pytest.mark.parametrize("shape", ALL, ids=PC.ids(ALL))
def test_weight_gradient_on_the_simulator(shape, monkeypatch):
    B, Cin, Cout, H, W, s = shape
    (x, dy, _), (ref64, yard, S), _ = case(shape)
    got, ws = _orders(monkeypatch, lambda fill: HP.wrw(x, dy, s, fill))
    assert got.dtype == np.float32 and got.shape == (Cout, Cin)
    ratio = PC.worst(torch.from_numpy(got.copy()).reshape(ref64.shape), ref64, yard, S)
    report(f"pw wrw on the simulator {shape}: {ws.size // (Cout * Cin)} partials, ATen fp32's max error {yard:.3e}, worst "
           f"entry at {ratio:.3f} of its bound")
    assert ratio <= 1.0, (shape, ratio)


@pytest.mark.parametrize("shape", PC.DGRAD_SHAPES, ids=PC.ids(PC.DGRAD_SHAPES))
def test_data_gradient_on_the_simulator(shape, monkeypatch):
    B, Cin, Cout, H, W, s = shape
    (_, dy, w), _, (ref64, yard, S) = case(shape)
    (got,) = _orders(monkeypatch, lambda fill: (HP.dgrad(dy, w, H, W, fill),))
    assert got.dtype == np.float32 and got.shape == (B, Cin, H, W)
    got = torch.from_numpy(got.copy())
    ratio = PC.worst(got, ref64, yard, S)
    report(f"pw dgrad on the simulator {shape}: ATen fp32's max error {yard:.3e}, worst entry at {ratio:.3f} of its bound")
    assert ratio <= 1.0, (shape, ratio)
    zeros = PC.unsampled(got)
    assert bool((zeros == 0).all()) and not bool(torch.signbit(zeros).any()), "a skipped position is not an exact +0"


@pytest.mark.parametrize("shape", ALL, ids=PC.ids(ALL))
def test_ternary_inputs_give_the_fp64_result_exactly(shape):
    """zero tolerance: with operands from {-1, 0, 1} no sum the kernels form is ever rounded"""
    B, Cin, Cout, H, W, s = shape
    x, dy, w = PC.operands(shape, ternary=True)
    got, _ = HP.wrw(x.numpy(), dy.numpy(), s)
    want = PC.aten_wgrad(x.double(), dy.double(), s).reshape(Cout, Cin)
    assert torch.equal(torch.from_numpy(got.copy()).double(), want), shape
    if s == 2:
        got = HP.dgrad(dy.numpy(), w.reshape(Cout, Cin).numpy(), H, W)
        assert torch.equal(torch.from_numpy(got.copy()).double(), PC.aten_dgrad(dy.double(), w.double(), H, W)), shape


def test_the_shapes_cover_what_the_kernels_distinguish():
    parts = lambda s: HP.ws_bytes(*s) // (4 * s[1] * s[2])  # noqa: E731
    chunks = lambda s: s[0] * -(-(PC.out_size(s[3], s[5]) * PC.out_size(s[4], s[5])) // 32)  # noqa: E731
    assert {(s[1], s[2]) for s in ALL} >= {(64, 128), (128, 256), (256, 512), (512, 256)}
    assert all(parts(s) == chunks(s) for s in PC.SHAPES) and parts((5, 64, 128, 9, 67, 2)) == 30
    assert all(chunks(s) > parts(s) == 32 for s in PC.MULTI)                 # some workgroups walk two chunks
    assert any(s[3] % 2 and s[4] % 2 for s in PC.DGRAD_SHAPES)               # the 2 x 2 cell cut at H and at W
    assert any(PC.out_size(s[3], 2) * PC.out_size(s[4], 2) < 4 for s in PC.DGRAD_SHAPES)
    assert any(s[0] * PC.out_size(s[3], 2) * PC.out_size(s[4], 2) > 64 for s in PC.DGRAD_SHAPES)  # several pixel tiles


def test_rejected_arguments_write_nothing():
    shape = (2, 64, 128, 6, 10, 2)
    (x, dy, w), _, _ = case(shape)
    k = HP._Call()
    xa, dya, wa = k.arg(x), k.arg(dy), k.arg(w)
    n = HP.ws_bytes(*shape)
    dw, ws, dx = k.out((128, 64), np.nan), k.out((n // 4,), np.nan), k.out((2, 64, 6, 10), np.nan)
    p = HP._ptr
    for args in ((2, 64, 128, 6, 10, 2, p(xa), p(dya), p(dw), p(ws), n - 4, None),
                 (2, 48, 128, 6, 10, 2, p(xa), p(dya), p(dw), p(ws), n, None),
                 (2, 64, 128, 6, 10, 3, p(xa), p(dya), p(dw), p(ws), n, None),
                 (2, 64, 128, 6, 10, 2, None, p(dya), p(dw), p(ws), n, None),
                 (2, 64, 128, 6, 10, 2, p(xa), p(dya), p(dw), None, n, None)):
        k.run("scsfm_pw_wrw_f32", *args, status=-1)
    for args in ((2, 64, 96, 6, 10, p(dya), p(wa), p(dx), None), (0, 64, 128, 6, 10, p(dya), p(wa), p(dx), None),
                 (2, 64, 128, 6, 10, p(dya), None, p(dx), None)):
        k.run("scsfm_pw_dgrad_f32", *args, status=-1)
    assert np.isnan(dw).all() and np.isnan(ws).all() and np.isnan(dx).all()
