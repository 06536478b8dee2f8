"""The data gradient of the decoder's low-channel 3x3 convolutions (csrc_dgrad/scsfm_conv_dgrad.hip) on the host
simulator (tests/_hostsim_dgrad.py; tests/hostsim/wrw_shim.h supplies the matrix instruction): 16 -> 16 at 1 x 1, 5 x 7
and 17 x 67 (3 x 2 tiles of 8 x 64 with partial ones, two images), 32 -> 16 at 9 x 70 (the padded grid is 11 x 72: two
tiles each way).  Per entry

    |dx32 - dx64| <= 2 max|aten32 - dx64| + 8 u S,     S = the same sum on absolute values in fp64, u = 2^-24

with ATen's convolution_backward as yardstick; inputs from {-1, 0, 1} must give the fp64 result to the bit; an impulse of
dy over weights of distinct integer codes must return the weight window at its place and zero elsewhere.  Every case
runs twice, in both thread orders, with two prefills of dx, between NaN guard bands.  The grid is one workgroup per
tile and is not capped, so no workgroup walks a second tile."""
import numpy as np
import pytest
import torch

import _hostsim_dgrad as HD
from _util import report
from test_dgrad_hostsim import both_orders_and_fills

U = 2.0 ** -24
# (B, Cin, Cout, H, W)
SHAPES = [(1, 16, 16, 1, 1), (2, 16, 16, 5, 7), (2, 16, 16, 17, 67), (1, 32, 16, 9, 70)]
_ids = ["x".join(map(str, s)) for s in SHAPES]


def aten_dgrad(dy, w):
    B, Cout, H, W = dy.shape
    x = torch.zeros(B, w.shape[1], H + 2, W + 2, dtype=dy.dtype)
    return torch.ops.aten.convolution_backward(dy, x, w, None, [1, 1], [0, 0], [1, 1], False, [0, 0], 1,
                                               [True, False, False])[0]


@pytest.mark.parametrize("order", ["forward", "reverse"])
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_data_gradient_on_the_simulator(shape, order, monkeypatch):
    B, Cin, Cout, H, W = shape
    gen = torch.Generator().manual_seed(sum(shape))
    dy, w = torch.randn(B, Cout, H, W, generator=gen), torch.randn(Cout, Cin, 3, 3, generator=gen)
    (dx,) = both_orders_and_fills(lambda fill: (HD.conv3x3_dgrad(dy.numpy(), w.numpy(), fill),), order, monkeypatch)
    dx64, S = aten_dgrad(dy.double(), w.double()), aten_dgrad(dy.double().abs(), w.double().abs())
    yard = float((aten_dgrad(dy, w).double() - dx64).abs().max())
    ratio = float(((torch.from_numpy(dx).double() - dx64).abs() / (2 * yard + 8 * U * S + 1e-300)).max())
    assert not np.isnan(dx).any() and ratio <= 1.0, (shape, ratio)
    report(f"data gradient on the simulator {shape} {order}: worst entry at {ratio:.3f} of the bound")


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_exact_inputs_and_impulses(shape):
    B, Cin, Cout, H, W = shape
    rng = np.random.default_rng(sum(shape))
    dy = rng.choice(np.array([-1, 0, 1], np.float32), (B, Cout, H, W))
    w = rng.choice(np.array([-1, 0, 1], np.float32), (Cout, Cin, 3, 3))
    dx = HD.conv3x3_dgrad(dy, w)
    want = aten_dgrad(torch.from_numpy(dy).double(), torch.from_numpy(w).double()).numpy()
    assert np.array_equal(dx.astype(np.float64), want)
    codes = (1 + np.arange(Cout * Cin * 9, dtype=np.float32)).reshape(Cout, Cin, 3, 3)
    for co in (0, 5, Cout - 1):
        for i, j in {(0, 0), (H - 1, W - 1), (H // 2, W // 2), (min(7, H - 1), min(63, W - 1)), (H - 1, min(64, W - 1))}:
            dy = np.zeros((B, Cout, H, W), np.float32)
            dy[B - 1, co, i, j] = 1
            dx = HD.conv3x3_dgrad(dy, codes)
            want = np.zeros_like(dx)
            want[B - 1, :, i:i + 3, j:j + 3] = codes[co]
            bad = np.argwhere(dx != want)
            assert not len(bad), (f"impulse at channel {co} pixel ({i}, {j}): {len(bad)} entries differ, first (n, ci, p, q) = "
                                  f"{tuple(bad[0])} holds {dx[tuple(bad[0])]} for {want[tuple(bad[0])]} "
                                  f"(codes are 1 + (co * Cin + ci) * 9 + 3 r + s)")


def test_rejected_arguments_write_nothing():
    import ctypes
    dy, w = np.ones((2, 16, 4, 5), np.float32), np.ones((16, 16, 3, 3), np.float32)
    dx = np.full((2, 16, 6, 7), np.nan, np.float32)
    p = lambda a: ctypes.c_void_p(a.ctypes.data)  # noqa: E731
    fn = HD.lib()._fn["scsfm_dgrad_conv3x3_f32"]
    good = [2, 16, 16, 4, 5, p(dy), p(w), p(dx), None]
    for k, bad in ((0, 0), (1, 8), (1, 64), (2, 1), (2, 32), (3, 0), (4, -1), (5, None), (6, None), (7, None)):
        args = list(good)
        args[k] = bad
        assert fn(*args) == -1 and np.isnan(dx).all(), (k, bad)
    covers = HD.lib()._fn["scsfm_dgrad_conv3x3_covers"]
    assert [(ci, co) for ci in (8, 16, 32, 64) for co in (1, 16, 32) if covers(ci, co)] == [(16, 16), (32, 16)]
