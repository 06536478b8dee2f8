"""Which 1x1 convolutions take scsfm_hip.conv1x1.conv1x1, without a GPU: the routed triples on CUDA fp32 contiguous NCHW
tensors with grad mode on, and nothing else -- not CPU, fp64 or channels_last tensors, not a call under no_grad, not another
kernel size, stride, padding, dilation or group count, not with SCSFM_CONV1X1_BWD=0; the call sites keep the plain module
call on CPU; and module tree and state-dict keys of both nets are those of tests/golden/model_keys.json."""
import json
import os

import pytest
import torch
import torch.nn as nn

from _util import GOLDEN


class _Cuda:
    """what conv1x1.applies asks of a tensor, answering as a CUDA tensor would (there is no GPU here)"""

    def __init__(self, t, is_cuda=True):
        self._t, self.is_cuda = t, is_cuda
        self.dtype, self.shape = t.dtype, t.shape

    def dim(self):
        return self._t.dim()

    def numel(self):
        return self._t.numel()

    def is_contiguous(self):
        return self._t.is_contiguous()


class _M:
    def __init__(self, conv, cuda_bias=True):
        bias = None if conv.bias is None else _Cuda(conv.bias.detach(), cuda_bias)
        self.__dict__.update(weight=_Cuda(conv.weight.detach()), bias=bias, stride=conv.stride, padding=conv.padding,
                             dilation=conv.dilation, groups=conv.groups, padding_mode=conv.padding_mode)


def _case(cin=64, cout=128, stride=2, dtype=torch.float32, channels_last=False, cpu=False, k=1, cuda_bias=True, **kw):
    conv = nn.Conv2d(cin, cout, k, stride, **kw).to(dtype)
    x = torch.randn(2, cin, 6, 10, dtype=dtype)
    if channels_last:
        x = x.contiguous(memory_format=torch.channels_last)
    return _Cuda(x, not cpu), _M(conv, cuda_bias)


@pytest.fixture
def pw_on(monkeypatch):
    from scsfm_hip import config
    monkeypatch.delenv("SCSFM_CONV1X1_BWD", raising=False)
    config.set_conv1x1_bwd(None)
    yield config
    config.set_conv1x1_bwd(None)


def test_only_routed_cuda_fp32_contiguous_1x1_convolutions_apply(pw_on, monkeypatch):
    from scsfm_hip import conv1x1 as PW
    every = {(64, 128, 2), (128, 256, 2), (256, 512, 2), (512, 256, 1)}
    assert PW.ROUTED <= every and PW.ROUTED_DGRAD <= {t for t in PW.ROUTED if t[2] == 2}
    assert all(PW.covers(*t) for t in every) and all(PW.dgrad_covers(*t) == (t[2] == 2) for t in every)
    monkeypatch.setattr(PW, "ROUTED", set(every))
    for cin, cout, s in sorted(every):
        assert PW.applies(*_case(cin, cout, s)), (cin, cout, s)
        assert PW.applies(*_case(cin, cout, s, bias=False))
    assert not PW.applies(*_case(cpu=True))
    assert not PW.applies(*_case(dtype=torch.float64))
    assert not PW.applies(*_case(channels_last=True))
    assert not PW.applies(*_case(cuda_bias=False))
    for cin, cout, s in ((64, 128, 1), (512, 256, 2), (256, 6, 1), (64, 256, 1), (256, 1024, 2), (64, 64, 1)):
        assert not PW.applies(*_case(cin, cout, s)), (cin, cout, s)   # net.3, ResNet-50's, foreign
    assert not PW.applies(*_case(k=3)) and not PW.applies(*_case(k=3, padding=1)) and not PW.applies(*_case(padding=1))
    assert not PW.applies(*_case(groups=2)) and not PW.applies(*_case(dilation=2)) and not PW.applies(*_case(stride=3))
    x, m = _case()
    assert PW.applies(x, m)
    with torch.no_grad():
        assert not PW.applies(x, m)
    monkeypatch.setattr(PW, "ROUTED", every - {(64, 128, 2)})
    assert not PW.applies(x, m)


def test_the_switch(pw_on, monkeypatch):
    from scsfm_hip import conv1x1 as PW
    monkeypatch.setattr(PW, "ROUTED", {(64, 128, 2)})
    x, m = _case()
    assert pw_on.conv1x1_bwd() and PW.applies(x, m)
    pw_on.set_conv1x1_bwd(False)
    assert not PW.applies(x, m)
    pw_on.set_conv1x1_bwd(None)
    monkeypatch.setenv("SCSFM_CONV1X1_BWD", "0")
    assert not pw_on.conv1x1_bwd() and not PW.applies(x, m)
    monkeypatch.setenv("SCSFM_CONV1X1_BWD", "1")
    assert not pw_on.conv1x1_bwd()  # (read once)
    pw_on.set_conv1x1_bwd(None)
    assert pw_on.conv1x1_bwd() and PW.applies(x, m)


def _refuse(*a, **k):
    raise AssertionError("conv1x1 was reached")


@pytest.mark.parametrize("variant", ["cpu_fp32", "cpu_fp64", "channels_last", "eval_no_grad"])
def test_cpu_fp64_and_channels_last_keep_the_module_call(variant, pw_on, monkeypatch):
    """both call sites, on tensors that never qualify: the nets compute what their reference chains compute, to the bit,
    and the autograd function is never built"""
    import models
    from scsfm_hip import conv1x1 as PW
    monkeypatch.setattr(PW, "conv1x1", _refuse)
    monkeypatch.setattr(PW._Conv1x1, "apply", _refuse)
    dtype = torch.float64 if variant == "cpu_fp64" else torch.float32
    torch.manual_seed(0)
    net = models.PoseResNet(18, False).to(dtype)
    a, b = torch.randn(2, 3, 32, 64, dtype=dtype), torch.randn(2, 3, 32, 64, dtype=dtype)
    if variant == "channels_last":
        net = net.to(memory_format=torch.channels_last)
        a, b = (t.contiguous(memory_format=torch.channels_last) for t in (a, b))
    if variant == "eval_no_grad":
        net.eval()
        with torch.no_grad():
            got = net(a, b)
            feats = net.encoder.forward_reference(torch.cat([a, b], 1))
    else:
        state = {k: v.clone() for k, v in net.state_dict().items()}
        got = net(a, b)
        net.load_state_dict(state)
        feats = net.encoder.forward_reference(torch.cat([a, b], 1))
    d = net.decoder
    out = d.relu(d.net[0](feats[-1]))
    out = d.net[3](d.relu(d.net[2](d.relu(d.net[1](out)))))
    assert torch.equal(got, 0.01 * out.mean(3).mean(2).view(-1, 6))


def test_conv_picks_the_function_where_it_applies(pw_on, monkeypatch):
    from scsfm_hip import conv1x1 as PW
    taken = []
    monkeypatch.setattr(PW, "applies", lambda x, m: True)
    monkeypatch.setattr(PW, "conv1x1", lambda x, w, b, s: taken.append((w.shape, b is None, s)) or "y")
    m = nn.Conv2d(64, 128, 1, 2, bias=False)
    assert PW.conv(m, torch.randn(1, 64, 2, 2)) == "y" and taken == [(m.weight.shape, True, 2)]
    monkeypatch.setattr(PW, "applies", lambda x, m: False)
    x = torch.randn(1, 64, 2, 2)
    assert torch.equal(PW.conv(m, x), m(x)) and len(taken) == 1


def test_the_down_sample_branch_asks_only_beside_the_projects_own_glue(monkeypatch):
    """_downsample hands the convolution to conv1x1.conv for a BatchNorm in training mode or a frozen one with the frozen
    path enabled; a module merely in eval mode, a frozen one under SCSFM_FROZEN_TORCH=1 and CPU tensors keep the module
    call"""
    from models import resnet_encoder as RE
    from scsfm_hip import conv1x1 as PW, encoder_frozen as EF
    asked = []
    real = torch.randn(2, 64, 6, 10)

    class OnDevice:  # (what _downsample reads of x before it hands it on)
        is_cuda = True

    monkeypatch.setattr(PW, "conv", lambda m, x: asked.append(1) or m(real))
    monkeypatch.delenv("SCSFM_FROZEN_TORCH", raising=False)
    ds = nn.Sequential(nn.Conv2d(64, 128, 1, 2, bias=False), nn.BatchNorm2d(128)).train()
    want = ds(real)
    assert torch.equal(RE._downsample(ds, OnDevice()), want) and asked == [1]
    assert torch.equal(RE._downsample(ds, real), ds(real)) and asked == [1]           # a CPU tensor
    ds.eval()
    del asked[:]
    monkeypatch.setattr(ds[0], "forward", lambda x: nn.Conv2d.forward(ds[0], real))
    assert torch.equal(RE._downsample(ds, OnDevice()), ds[1](nn.Conv2d.forward(ds[0], real))) and not asked  # eval mode
    assert EF.freeze(ds) == 1 and not ds.train()[1].training
    RE._downsample(ds, OnDevice())
    assert asked == [1]                                                               # frozen: asked
    monkeypatch.setenv("SCSFM_FROZEN_TORCH", "1")
    RE._downsample(ds, OnDevice())
    assert asked == [1]                                                               # ... unless sent down ATen


def test_the_function_on_cpu_is_the_convolution(pw_on, monkeypatch):
    """the node itself, off the routed sets: forward F.conv2d's bits, every gradient ATen's, frozen inputs get None"""
    import torch.nn.functional as F
    from scsfm_hip import conv1x1 as PW
    monkeypatch.setattr(PW, "ROUTED", set())
    monkeypatch.setattr(PW, "ROUTED_DGRAD", set())
    monkeypatch.setattr(PW, "weight_grad", _refuse)
    monkeypatch.setattr(PW, "data_grad", _refuse)
    g = torch.Generator().manual_seed(2)
    x = torch.randn(2, 64, 5, 7, generator=g, requires_grad=True)
    w = torch.randn(128, 64, 1, 1, generator=g, requires_grad=True)
    b = torch.randn(128, generator=g, requires_grad=True)
    gy = torch.randn(2, 128, 3, 4, generator=g)
    y, y_ref = PW.conv1x1(x, w, b, 2), F.conv2d(x, w, b, 2)
    assert torch.equal(y, y_ref)
    for got, want in zip(torch.autograd.grad(y, (x, w, b), gy), torch.autograd.grad(y_ref, (x, w, b), gy)):
        assert torch.allclose(got, want, rtol=1e-5, atol=1e-5)
    (gw,) = torch.autograd.grad(PW.conv1x1(x.detach(), w, None, 2), (w,), gy)
    assert gw.shape == w.shape and not PW.conv1x1(x.detach(), w.detach(), None, 2).requires_grad


@pytest.mark.parametrize("layers", [18, 50])
def test_state_dict_and_module_tree_unchanged(layers):
    import models
    want = json.load(open(os.path.join(GOLDEN, "model_keys.json")))
    torch.manual_seed(0)
    for name, net in ((f"DispResNet{layers}", models.DispResNet(layers, False)),
                      (f"PoseResNet{layers}", models.PoseResNet(layers, False))):
        assert [[k, list(v.shape)] for k, v in net.state_dict().items()] == want[name], name
    pose = models.PoseResNet(layers, False)
    assert [n for n, _ in pose.decoder.named_children()] == ["net", "relu"]
    assert isinstance(pose.encoder.encoder.layer2[0].downsample[0], nn.Conv2d)
