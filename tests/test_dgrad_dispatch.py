"""When the depth decoder's full-resolution tail takes scsfm_hip.decoder_dgrad.head_tail, without a GPU: never on CPU,
fp64 or channels_last tensors, for another channel count or a head that is no plain 3x3 convolution, or with
SCSFM_DECODER_DGRAD=0; and, with the host simulator (tests/_hostsim_dgrad.py) in place of libscsfm_dgrad.so, a whole
DepthDecoder forward and backward against the reference chain, its forward identical to the switched-off path."""
import copy

import pytest
import torch
import torch.nn as nn

import _hostsim_decb as HB
import _hostsim_dgrad as HD
import _hostsim_nets as HS
import _hostsim_wrw as HW
from _util import report


class _Cuda:
    """what decoder_dgrad.applies asks of a tensor, answering as a CUDA tensor would (there is no GPU here)"""

    def __init__(self, t, is_cuda=True):
        self._t, self.is_cuda = t, is_cuda
        self.dtype, self.shape = t.dtype, t.shape

    def dim(self):
        return self._t.dim()

    def is_contiguous(self):
        return self._t.is_contiguous()


class _M:
    def __init__(self, conv, is_cuda=True):
        self.__dict__.update(weight=_Cuda(conv.weight.detach(), is_cuda),
                             bias=None if conv.bias is None else _Cuda(conv.bias.detach(), is_cuda), stride=conv.stride,
                             padding=conv.padding, dilation=conv.dilation, groups=conv.groups,
                             padding_mode=conv.padding_mode)


def _case(C=16, cout=1, dtype=torch.float32, channels_last=False, cpu=False, size=(7, 9), **kw):
    head = nn.Conv2d(C, cout, kw.pop("k", 3), **kw).to(dtype)
    b = torch.randn(2, C, *size, dtype=dtype)
    if channels_last:
        b = b.contiguous(memory_format=torch.channels_last)
    return _Cuda(b, not cpu), _Cuda(torch.randn(C, dtype=dtype), not cpu), _M(head, not cpu)


@pytest.fixture
def dgrad_on(monkeypatch):
    from scsfm_hip import config
    monkeypatch.delenv("SCSFM_DECODER_DGRAD", raising=False)
    monkeypatch.delenv("SCSFM_DECODER_WRW", raising=False)
    config.set_decoder_dgrad(None)
    config.set_decoder_wrw(None)
    yield config
    config.set_decoder_dgrad(None)
    config.set_decoder_wrw(None)


def test_only_a_covered_cuda_fp32_contiguous_tail_applies(dgrad_on, monkeypatch):
    from scsfm_hip import decoder_dgrad as DG
    assert DG.applies(*_case()) and DG.applies(*_case(size=(2, 2)))
    assert not DG.applies(*_case(cpu=True))
    assert not DG.applies(*_case(dtype=torch.float64))
    assert not DG.applies(*_case(channels_last=True))
    for C in (8, 32, 64):
        assert not DG.applies(*_case(C)), C
    assert not DG.applies(*_case(cout=2)) and not DG.applies(*_case(bias=False))
    assert not DG.applies(*_case(stride=2)) and not DG.applies(*_case(padding=1)) and not DG.applies(*_case(dilation=2))
    assert not DG.applies(*_case(k=1)) and not DG.applies(*_case(size=(1, 9)))
    b, bias, head = _case()
    assert not DG.applies(b, None, head)
    dgrad_on.set_decoder_dgrad(False)
    assert not DG.applies(b, bias, head)
    dgrad_on.set_decoder_dgrad(None)
    monkeypatch.setenv("SCSFM_DECODER_DGRAD", "0")
    assert not dgrad_on.decoder_dgrad() and not DG.applies(b, bias, head)
    dgrad_on.set_decoder_dgrad(None)
    monkeypatch.setenv("SCSFM_DECODER_DGRAD", "1")
    assert dgrad_on.decoder_dgrad() and DG.applies(b, bias, head)


def test_only_routed_cuda_fp32_contiguous_gradients_take_the_data_gradient(dgrad_on):
    from scsfm_hip import conv_wrw as CW
    gy = lambda **kw: _Cuda(torch.randn(2, 16, 5, 7, dtype=kw.get("dtype", torch.float32)), not kw.get("cpu"))  # noqa: E731
    w = lambda cin=16, cout=16: _Cuda(torch.randn(cout, cin, 3, 3))  # noqa: E731
    assert all(CW.dgrad_covers(*p) for p in CW.ROUTED_DGRAD)
    for cin, cout in CW.ROUTED_DGRAD:
        assert CW.data_grad_routed(gy(), w(cin, cout))
    assert not CW.data_grad_routed(gy(cpu=True), w()) and not CW.data_grad_routed(gy(dtype=torch.float64), w())
    assert not CW.data_grad_routed(gy(), w(64, 32)) and not CW.data_grad_routed(gy(), w(96, 32))
    assert not CW.data_grad_routed(_Cuda(torch.randn(2, 16, 5, 7).contiguous(memory_format=torch.channels_last)), w())
    dgrad_on.set_decoder_dgrad(False)
    assert not CW.data_grad_routed(gy(), w())


def test_the_data_gradient_does_not_depend_on_the_weight_gradient_switch(dgrad_on):
    """with SCSFM_DECODER_WRW=0 the routed layers take conv3x3_valid(..., wrw=False) (applies_without_wrw), so that their input
    gradients are the same kernel's with the weight-gradient switch on and off"""
    from scsfm_hip import conv_wrw as CW

    def case(cin, cout, cpu=False, **kw):
        conv = nn.Conv2d(cin, cout, kw.pop("k", 3), **kw)
        return _Cuda(torch.randn(2, cin, 7, 9), not cpu), _M(conv)
    for on in (True, False):
        dgrad_on.set_decoder_wrw(on)
        for cin, cout in sorted(CW.ROUTED):
            assert CW.applies(*case(cin, cout)) == on
            assert CW.applies_without_wrw(*case(cin, cout)) == ((cin, cout) in CW.ROUTED_DGRAD)
        assert not CW.applies_without_wrw(*case(16, 16, cpu=True)) and not CW.applies_without_wrw(*case(16, 16, padding=1))
        assert not CW.applies_without_wrw(*case(16, 16, k=1)) and not CW.applies_without_wrw(*case(64, 16))
    dgrad_on.set_decoder_dgrad(False)
    assert not CW.applies_without_wrw(*case(16, 16))


def _refuse(*a, **k):
    raise AssertionError("the tail-backward library was reached")


@pytest.mark.parametrize("variant", ["cpu_fp32", "cpu_fp64", "channels_last"])
def test_cpu_fp64_and_channels_last_never_reach_the_library(variant, dgrad_on, monkeypatch):
    import models
    from scsfm_hip import _lib, conv_wrw as CW, decoder_dgrad as DG
    monkeypatch.setattr(CW, "data_grad", _refuse)
    monkeypatch.setattr(DG._HeadTail, "apply", _refuse)
    monkeypatch.setattr(DG, "tail_bwd", _refuse)
    monkeypatch.setattr(_lib, "get_dgrad", _refuse)
    dtype = torch.float64 if variant == "cpu_fp64" else torch.float32
    torch.manual_seed(0)
    net = models.DispResNet(18, False).to(dtype).train()
    x = torch.randn(1, 3, 64, 96, dtype=dtype)
    if variant == "channels_last":
        net, x = net.to(memory_format=torch.channels_last), x.contiguous(memory_format=torch.channels_last)
    sum(o.sum() for o in net(x)).backward()
    assert all(p.grad is not None for p in net.decoder.parameters())


# ------------------------------------------------------------------ the whole decoder over the simulator, on the CPU

NUM_CH_ENC = [4, 4, 8, 8, 16]
VARIANTS = [((2, 3), sc, al) for sc in (range(4), [0, 2]) for al in (False, True)] + [((2, 17), range(4), False)]


def _features(h, w, dtype=torch.float32):
    g = torch.Generator().manual_seed(100 * h + w)
    return [torch.randn(2, c, h << (4 - k), w << (4 - k), generator=g).to(dtype) for k, c in enumerate(NUM_CH_ENC)]


def _decoder_run(dec, feats, weights, num_scales, fused):
    feats = [f.clone().requires_grad_() for f in feats]
    outs = dec.forward_fused_bias(feats) if fused else dec.forward_reference(feats)
    loss = sum((o * w.to(o.dtype)).sum() for o, w in zip(outs[:num_scales], weights))
    grads = torch.autograd.grad(loss, feats + list(dec.parameters()), allow_unused=True)
    return [o.detach() for o in outs] + list(grads)


@pytest.mark.parametrize("size,scales,all_scales", VARIANTS, ids=[
    f"{h}x{w}-heads{''.join(map(str, sc))}-{'all_scales' if al else 'one_scale'}" for (h, w), sc, al in VARIANTS])
def test_the_whole_decoder_with_the_simulated_tail(size, scales, all_scales, dgrad_on, monkeypatch):
    """forward_fused_bias with the glue, the routed weight and data gradients and the tail on the simulator against
    forward_reference in fp32 and fp64, under the bound of tests/test_decbias_hostsim.py: for every output, feature
    gradient and parameter gradient  max|new32 - ref64| <= 2 max|ref32 - ref64| + 1e-7 max|ref64|.  The tail runs once
    and the data gradient once per routed layer; switched off neither runs, the forward keeps its bits and the gradients
    stay under the same bound."""
    from models.DispResNet import DepthDecoder
    from scsfm_hip import conv_wrw as CW, decoder as D, decoder_bias as DB, decoder_dgrad as DG
    monkeypatch.setattr(D, "pad", HS.pad)
    for name in ("elu_pad", "up_cat_pad", "disp_head"):
        monkeypatch.setattr(DB, name, getattr(HB, name))
    real_cw, real_dg = CW.applies, DG.applies
    monkeypatch.setattr(CW, "applies", lambda x, m: real_cw(_Cuda(x), _M(m)))
    monkeypatch.setattr(CW, "weight_grad", HW.weight_grad)
    monkeypatch.setattr(DG, "applies", lambda b, bias, head: real_dg(_Cuda(b), _Cuda(bias), _M(head)))
    monkeypatch.setattr(DG, "head_tail", HD.head_tail)
    monkeypatch.setattr(DG, "tail_bwd", _refuse)
    real_da = CW.data_grad_routed
    monkeypatch.setattr(CW, "data_grad_routed", lambda gy, w: real_da(_Cuda(gy), _Cuda(w)))
    monkeypatch.setattr(CW, "data_grad", HD.data_grad)
    torch.manual_seed(7)
    dec = DepthDecoder(NUM_CH_ENC, scales=scales).float()
    dec64 = copy.deepcopy(dec).double()
    feats = _features(*size)
    assert not dec.fused_path_applies(feats)
    n_out = len(list(scales))
    g = torch.Generator().manual_seed(11)
    weights = [torch.rand(2, 1, (size[0] << 5) >> s, (size[1] << 5) >> s, generator=g) + 0.5 for s in list(scales)]
    num_scales = n_out if all_scales else 1
    HD.CALLS[0] = 0
    del HD.DATA_GRAD_CALLS[:]
    new = _decoder_run(dec, feats, weights, num_scales, True)
    assert HD.CALLS[0] == 1 and sorted(HD.DATA_GRAD_CALLS) == [(16, 16), (32, 16)] == sorted(CW.ROUTED_DGRAD)
    ref32 = _decoder_run(dec, feats, weights, num_scales, False)
    ref64 = _decoder_run(dec64, [f.double() for f in feats], weights, num_scales, False)
    dgrad_on.set_decoder_dgrad(False)
    off = _decoder_run(dec, feats, weights, num_scales, True)
    assert HD.CALLS[0] == 1 and len(HD.DATA_GRAD_CALLS) == 2
    assert len(new) == len(off) == len(ref32) == len(ref64) == n_out + 5 + len(list(dec.parameters()))
    for k in range(n_out):
        assert torch.equal(new[k], off[k]), f"output {k} changes with the switch"
    worst, used = 0.0, 0
    for k, (a, o, b, c) in enumerate(zip(new, off, ref32, ref64)):
        assert (a is None) == (o is None) == (b is None) == (c is None), k
        if a is None:
            continue
        used += 1
        assert a.shape == c.shape and a.dtype == torch.float32, k
        yard, scale = float((b.double() - c).abs().max()), float(c.abs().max())
        for t in (a, o):
            err = float((t.double() - c).abs().max())
            assert err <= 2 * yard + 1e-7 * scale, (k, tuple(a.shape), err, yard, scale)
        worst = max(worst, float((a.double() - c).abs().max()) / (yard + 0.5e-7 * scale + 1e-300))
    assert used > n_out + 1
    report(f"decoder with the simulated tail {size} heads={list(scales)} num_scales={num_scales}: at {worst:.2f} x the "
           f"fp32 reference chain's own error ({used} tensors)")
