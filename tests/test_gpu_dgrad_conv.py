"""The data gradient of the decoder's low-channel 3x3 convolutions (scsfm_hip.conv_wrw.data_grad,
csrc_dgrad/scsfm_conv_dgrad.hip) on the GPU, at the shapes of tests/test_dgrad_conv_hostsim.py and under its bound, with
MIOpen's fp32 data gradient as yardstick: per entry |dx32 - dx64| <= 2 max|miopen32 - dx64| + 8 u S.  Inputs from
{-1, 0, 1} must give the fp64 result to the bit, an impulse of dy over coded weights must return the weight window (which
confirms the lane maps on the real matrix instruction), a second call gives the same bits, and operands that are views
between NaN give the bits of fresh copies."""
import numpy as np
import pytest
import torch

from _util import report
from test_dgrad_conv_hostsim import SHAPES, U, _ids

pytestmark = pytest.mark.gpu

DEV = "cuda"


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def aten_dgrad(dy, w):
    B, Cout, H, W = dy.shape
    x = torch.zeros(B, w.shape[1], H + 2, W + 2, dtype=dy.dtype, device=dy.device)
    return torch.ops.aten.convolution_backward(dy, x, w, None, [1, 1], [0, 0], [1, 1], False, [0, 0], 1,
                                               [True, False, False])[0]


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_data_gradient_against_fp64_and_miopen(shape):
    from scsfm_hip import conv_wrw as CW
    B, Cin, Cout, H, W = shape
    gen = torch.Generator(device=DEV).manual_seed(sum(shape))
    dy = torch.randn(B, Cout, H, W, device=DEV, generator=gen)
    w = torch.randn(Cout, Cin, 3, 3, device=DEV, generator=gen)
    dx = CW.data_grad(dy, w)
    assert same_bits(dx, CW.data_grad(dy, w)), "a second call gives other bits"
    dx64, S = aten_dgrad(dy.double(), w.double()), aten_dgrad(dy.double().abs(), w.double().abs())
    yard = float((aten_dgrad(dy, w).double() - dx64).abs().max())
    ratio = float(((dx.double() - dx64).abs() / (2 * yard + 8 * U * S + 1e-300)).max())
    assert bool(torch.isfinite(dx).all()) and ratio <= 1.0, (shape, ratio)
    report(f"data gradient on the GPU {shape}: worst entry at {ratio:.3f} of the bound")


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_exact_inputs_and_impulses(shape):
    from scsfm_hip import conv_wrw as CW
    B, Cin, Cout, H, W = shape
    gen = torch.Generator(device=DEV).manual_seed(sum(shape))
    dy = torch.randint(-1, 2, (B, Cout, H, W), device=DEV, generator=gen).float()
    w = torch.randint(-1, 2, (Cout, Cin, 3, 3), device=DEV, generator=gen).float()
    assert torch.equal(CW.data_grad(dy, w).double(), aten_dgrad(dy.double(), w.double()))
    codes = (1 + torch.arange(Cout * Cin * 9, dtype=torch.float32, device=DEV)).reshape(Cout, Cin, 3, 3)
    for co in (0, 5, Cout - 1):
        for i, j in {(0, 0), (H - 1, W - 1), (H // 2, W // 2), (min(7, H - 1), min(63, W - 1)), (H - 1, min(64, W - 1))}:
            dy = torch.zeros(B, Cout, H, W, device=DEV)
            dy[B - 1, co, i, j] = 1
            dx = CW.data_grad(dy, codes).cpu().numpy()
            want = np.zeros_like(dx)
            want[B - 1, :, i:i + 3, j:j + 3] = codes[co].cpu().numpy()
            bad = np.argwhere(dx != want)
            assert not len(bad), (f"impulse at channel {co} pixel ({i}, {j}): {len(bad)} entries differ, first (n, ci, p, q) "
                                  f"= {tuple(bad[0])} holds {dx[tuple(bad[0])]} for {want[tuple(bad[0])]}")


@pytest.mark.parametrize("offset", [1, 1029])
def test_operands_that_are_views_between_nan(offset):
    from scsfm_hip import conv_wrw as CW
    gen = torch.Generator(device=DEV).manual_seed(offset)
    dy0 = torch.randn(2, 16, 17, 67, device=DEV, generator=gen)
    w0 = torch.randn(16, 32, 3, 3, device=DEV, generator=gen)
    want = CW.data_grad(dy0, w0)

    def between_nan(t):
        flat = torch.full((offset + t.numel() + 1031,), float("nan"), device=DEV)
        v = flat[offset:offset + t.numel()].view(t.shape)
        v.copy_(t)
        assert v.is_contiguous() and v.data_ptr() % 16 != 0
        return flat, v

    (df, dy), (wf, w) = between_nan(dy0), between_nan(w0)
    got = CW.data_grad(dy, w)
    assert bool(torch.isfinite(got).all()) and same_bits(got, want)
    for flat, t in ((df, dy0), (wf, w0)):
        assert bool(torch.isnan(flat[:offset]).all()) and bool(torch.isnan(flat[offset + t.numel():]).all())


def test_conv3x3_valid_takes_the_routed_input_gradients():
    """with the switch on the input gradient of a routed layer is data_grad's, to the bit, and one call; switched off it
    is MIOpen's and the kernel is not called; a frozen input costs no launch"""
    import torch.nn.functional as F

    from scsfm_hip import config, conv_wrw as CW
    gen = torch.Generator(device=DEV).manual_seed(3)
    for cin, cout in sorted(CW.ROUTED_DGRAD):
        x = torch.randn(2, cin, 11, 37, device=DEV, generator=gen, requires_grad=True)
        w = torch.randn(cout, cin, 3, 3, device=DEV, generator=gen, requires_grad=True)
        gy = torch.randn(2, cout, 9, 35, device=DEV, generator=gen)
        calls, real = [], CW.data_grad
        try:
            CW.data_grad = lambda *a: calls.append(1) or real(*a)
            (gx,) = torch.autograd.grad(CW.conv3x3_valid(x, w), (x,), gy)
            assert calls == [1] and same_bits(gx, real(gy, w.detach()))
            torch.autograd.grad(CW.conv3x3_valid(x.detach(), w), (w,), gy)
            assert calls == [1]
            config.set_decoder_dgrad(False)
            (gx_off,) = torch.autograd.grad(CW.conv3x3_valid(x, w), (x,), gy)
            assert calls == [1]
        finally:
            CW.data_grad = real
            config.set_decoder_dgrad(None)
        (gx_ref,) = torch.autograd.grad(F.conv2d(x, w), (x,), gy)
        assert float((gx_off - gx_ref).abs().max()) <= 1e-5 * float(gx_ref.abs().max())
        assert float((gx - gx_ref).abs().max()) <= 1e-5 * float(gx_ref.abs().max())
