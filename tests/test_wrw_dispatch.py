"""Which convolutions of the depth decoder take scsfm_hip.conv_wrw.conv3x3_valid, without a GPU: none on CPU, fp64 or
channels_last tensors, for channel counts outside the routed set, or with SCSFM_DECODER_WRW=0; and, with the host
simulator's weight gradient (tests/_hostsim_wrw.py) in place of libscsfm_wrw.so, a whole DepthDecoder forward and
backward against the reference chain."""
import copy

import pytest
import torch
import torch.nn as nn

import _hostsim_decb as HB
import _hostsim_nets as HS
import _hostsim_wrw as HW
from _util import report

U = 2.0 ** -24


class _Cuda:
    """what conv_wrw.applies asks of a tensor, answering as a CUDA tensor would (there is no GPU here)"""

    def __init__(self, t, is_cuda=True):
        self._t, self.is_cuda = t, is_cuda
        self.dtype, self.shape = t.dtype, t.shape

    def dim(self):
        return self._t.dim()

    def is_contiguous(self):
        return self._t.is_contiguous()


class _M:
    def __init__(self, conv):
        self.__dict__.update(weight=_Cuda(conv.weight.detach()), stride=conv.stride, padding=conv.padding,
                             dilation=conv.dilation, groups=conv.groups, padding_mode=conv.padding_mode)


def _case(cin=16, cout=16, dtype=torch.float32, channels_last=False, cpu=False, **kw):
    conv = nn.Conv2d(cin, cout, kw.pop("k", 3), **kw).to(dtype)
    x = torch.randn(2, cin, 7, 9, dtype=dtype)
    if channels_last:
        x = x.contiguous(memory_format=torch.channels_last)
    return _Cuda(x, not cpu), _M(conv)


@pytest.fixture
def wrw_on(monkeypatch):
    from scsfm_hip import config
    monkeypatch.delenv("SCSFM_DECODER_WRW", raising=False)
    config.set_decoder_wrw(None)
    yield config
    config.set_decoder_wrw(None)


def test_only_routed_cuda_fp32_contiguous_3x3_convolutions_apply(wrw_on, monkeypatch):
    from scsfm_hip import conv_wrw as CW
    for cin, cout in sorted(CW.ROUTED):
        assert CW.applies(*_case(cin, cout)), (cin, cout)
    assert not CW.applies(*_case(cpu=True))
    assert not CW.applies(*_case(dtype=torch.float64))
    assert not CW.applies(*_case(channels_last=True))
    for cin, cout in ((128, 1), (128, 64), (512, 256), (24, 16), (16, 8), (256, 128)):  # head 3, upper levels, foreign
        assert not CW.applies(*_case(cin, cout)), (cin, cout)
    assert not CW.applies(*_case(stride=2)) and not CW.applies(*_case(padding=1)) and not CW.applies(*_case(dilation=2))
    assert not CW.applies(*_case(k=1)) and not CW.applies(*_case(groups=2))
    x, m = _case()
    assert CW.applies(x, m)
    wrw_on.set_decoder_wrw(False)
    assert not CW.applies(x, m)
    wrw_on.set_decoder_wrw(None)
    monkeypatch.setenv("SCSFM_DECODER_WRW", "0")
    assert not wrw_on.decoder_wrw() and not CW.applies(x, m)
    wrw_on.set_decoder_wrw(None)
    monkeypatch.setenv("SCSFM_DECODER_WRW", "1")
    assert wrw_on.decoder_wrw() and CW.applies(x, m)


def _refuse(*a, **k):
    raise AssertionError("conv3x3_valid was reached")


@pytest.mark.parametrize("variant", ["cpu_fp32", "cpu_fp64", "channels_last"])
def test_cpu_fp64_and_channels_last_never_reach_the_kernel(variant, wrw_on, monkeypatch):
    import models
    from scsfm_hip import _lib, conv_wrw as CW
    monkeypatch.setattr(CW._Conv3x3Valid, "apply", _refuse)
    monkeypatch.setattr(CW, "weight_grad", _refuse)
    monkeypatch.setattr(_lib, "get_wrw", _refuse)
    dtype = torch.float64 if variant == "cpu_fp64" else torch.float32
    torch.manual_seed(0)
    net = models.DispResNet(18, False).to(dtype).train()
    x = torch.randn(1, 3, 64, 96, dtype=dtype)
    if variant == "channels_last":
        net, x = net.to(memory_format=torch.channels_last), x.contiguous(memory_format=torch.channels_last)
    sum(o.sum() for o in net(x)).backward()
    assert all(p.grad is not None for p in net.decoder.parameters())


# ------------------------------------------------------------------ the whole decoder over the simulator, on the CPU

NUM_CH_ENC = [64, 4, 8, 8, 16]  # (64 skip channels at level 1: conv (1, 1) is the 96 -> 32 layer)
# decoder.<k> of convs (1,0), (1,1), (0,0), (0,1) and of the heads of scales 0, 1, 2
ROUTED_KEYS = {6: (64, 32), 7: (96, 32), 8: (32, 16), 9: (16, 16), 10: (16, 1), 11: (32, 1), 12: (64, 1)}


def _features(h, w, dtype=torch.float32):
    g = torch.Generator().manual_seed(100 * h + w)
    return [torch.randn(1, c, h << (4 - k), w << (4 - k), generator=g).to(dtype) for k, c in enumerate(NUM_CH_ENC)]


def _decoder_run(dec, feats, weights, fused):
    feats = [f.clone().requires_grad_() for f in feats]
    outs = dec.forward_fused_bias(feats) if fused == "bias" else (dec.forward_fused(feats) if fused else
                                                                 dec.forward_reference(feats))
    loss = sum((o * w.to(o.dtype)).sum() for o, w in zip(outs, weights))
    names = [f"feat{k}" for k in range(5)] + [n for n, _ in dec.named_parameters()]
    grads = torch.autograd.grad(loss, feats + list(dec.parameters()))
    return dict([(f"out{k}", o.detach()) for k, o in enumerate(outs)] + list(zip(names, grads)))


@pytest.mark.parametrize("path", ["bias", "fused"])
def test_the_whole_decoder_with_the_simulated_weight_gradient(path, wrw_on, monkeypatch):
    """forward_fused_bias / forward_fused with the glue and the routed layers' weight gradients on the simulator against
    forward_reference in fp32 and fp64.  The routed weight gradients: per entry |new32 - ref64| <= 2 max|ref32 - ref64|
    + 8 u S, S = sum |dy| |x| of the tensors the kernel was given; every other output and gradient: the bound of
    tests/test_decbias_hostsim.py, max|new32 - ref64| <= 2 max|ref32 - ref64| + 1e-7 max|ref64|.  With the switch off
    the simulator is not called."""
    from models.DispResNet import DepthDecoder
    from scsfm_hip import conv_wrw as CW, decoder as D, decoder_bias as DB
    for name in ("pad", "up_cat_pad", "elu_pad"):
        monkeypatch.setattr(D, name, getattr(HS, name))
    for name in ("elu_pad", "up_cat_pad", "disp_head"):
        monkeypatch.setattr(DB, name, getattr(HB, name))
    S = {}

    def weight_grad(x, gy):
        w = torch.zeros(gy.shape[1], x.shape[1], 3, 3, dtype=torch.float64)
        S[(x.shape[1], gy.shape[1])] = torch.ops.aten.convolution_backward(
            gy.double().abs(), x.double().abs(), w, None, [1, 1], [0, 0], [1, 1], False, [0, 0], 1,
            [False, True, False])[1]
        return HW.weight_grad(x, gy)

    real = CW.applies
    monkeypatch.setattr(CW, "applies", lambda x, m: real(_Cuda(x), _M(m)))
    monkeypatch.setattr(CW, "weight_grad", weight_grad)
    torch.manual_seed(7)
    dec = DepthDecoder(NUM_CH_ENC).float()
    dec64 = copy.deepcopy(dec).double()
    feats = _features(2, 2)
    assert not dec.fused_path_applies(feats)
    g = torch.Generator().manual_seed(11)
    weights = [torch.rand(1, 1, 64 >> s, 64 >> s, generator=g) + 0.5 for s in range(4)]
    HW.CALLS[0] = 0
    new = _decoder_run(dec, feats, weights, path)
    assert HW.CALLS[0] == 7 and set(S) == set(ROUTED_KEYS.values()) == CW.ROUTED
    ref32 = _decoder_run(dec, feats, weights, False)
    ref64 = _decoder_run(dec64, [f.double() for f in feats], weights, False)
    assert list(new) == list(ref32) == list(ref64)
    routed = {f"decoder.{k}.conv.conv.weight" if k < 10 else f"decoder.{k}.conv.weight": key
              for k, key in ROUTED_KEYS.items()}
    assert set(routed) <= set(new)
    worst = 0.0
    for name in new:
        a, b, c = new[name], ref32[name], ref64[name]
        assert a.shape == c.shape and a.dtype == torch.float32, name
        err, yard, scale = (a.double() - c).abs(), float((b.double() - c).abs().max()), float(c.abs().max())
        if name in routed:
            bound = 2 * yard + 8 * U * S[routed[name]]
            assert bool((err <= bound).all()), (name, float((err / bound).max()))
            worst = max(worst, float((err / bound).max()))
        else:
            assert float(err.max()) <= 2 * yard + 1e-7 * scale, (name, float(err.max()), yard, scale)
    report(f"decoder ({path}) with the simulated weight gradient: the routed layers' worst entry at {worst:.3f} of its "
           f"bound")
    # switched off: the same path without a call of the kernel, and the same gradients as the reference chain allows
    wrw_on.set_decoder_wrw(False)
    off = _decoder_run(dec, feats, weights, path)
    assert HW.CALLS[0] == 7
    for name in routed:
        yard = float((ref32[name].double() - ref64[name]).abs().max())
        assert float((off[name] - new[name]).abs().max()) <= 4 * yard + 16 * U * float(S[routed[name]].max())
