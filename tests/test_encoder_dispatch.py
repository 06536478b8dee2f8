"""Which path the ResNet encoder takes without a GPU: CPU, fp64, channels_last and eval inputs run the ATen chain
(forward_reference) unchanged, and module tree / state-dict keys of both nets are those of tests/golden/model_keys.json."""
import json
import os

import pytest
import torch

from _util import GOLDEN


def _refuse(*a, **k):
    raise AssertionError("the fused path was taken")


@pytest.mark.parametrize("variant", ["cpu_fp32_train", "cpu_fp32_eval", "cpu_fp64", "channels_last"])
@pytest.mark.parametrize("layers", [18, 50])
def test_cpu_inputs_take_the_reference_chain(variant, layers, monkeypatch):
    from models.resnet_encoder import ResnetEncoder, _fused_applies
    from scsfm_hip import encoder as E
    monkeypatch.setattr(E, "bn_act", _refuse)
    monkeypatch.setattr(E, "max_pool", _refuse)
    dtype = torch.float64 if variant == "cpu_fp64" else torch.float32
    torch.manual_seed(0)
    enc = ResnetEncoder(layers, False).to(dtype)
    enc.train(variant != "cpu_fp32_eval")
    x = torch.randn(2, 3, 32, 64, dtype=dtype)
    if variant == "channels_last":
        enc, x = enc.to(memory_format=torch.channels_last), x.contiguous(memory_format=torch.channels_last)
    assert not _fused_applies(enc.encoder.conv1(x), enc.encoder.bn1)
    state = {k: v.clone() for k, v in enc.state_dict().items()}
    got = enc(x)
    after = {k: v.clone() for k, v in enc.state_dict().items()}
    enc.load_state_dict(state)
    ref = enc.forward_reference(x)
    assert len(got) == len(ref) == 5 and all(torch.equal(a, b) for a, b in zip(got, ref))
    assert all(torch.equal(after[k], v) for k, v in enc.state_dict().items())  # the same buffer updates


def test_what_disqualifies_a_batchnorm():
    """(on CPU tensors nothing qualifies; the module-side conditions are read off a stand-in that claims to be CUDA)"""
    from scsfm_hip import encoder as E
    import torch.nn as nn
    x = torch.randn(2, 4, 3, 3)
    assert not E.applies(x, nn.BatchNorm2d(4)) and not E.pool_applies(x)
    for bn in (nn.BatchNorm2d(4).eval(), nn.BatchNorm2d(4, momentum=None), nn.BatchNorm2d(4, affine=False),
               nn.BatchNorm2d(4, track_running_stats=False)):
        assert not E.applies(x, bn)
    with pytest.raises(ValueError):
        E.bn_act(x, nn.BatchNorm2d(4))
    with pytest.raises(ValueError):
        E.max_pool(x)


@pytest.mark.parametrize("layers", [18, 50])
def test_state_dict_keys_are_the_goldens(layers):
    import models
    want = json.load(open(os.path.join(GOLDEN, "model_keys.json")))
    torch.manual_seed(0)
    for name, net in ((f"DispResNet{layers}", models.DispResNet(layers, False)),
                      (f"PoseResNet{layers}", models.PoseResNet(layers, False))):
        have = [[k, list(v.shape)] for k, v in net.state_dict().items()]
        assert have == want[name], name
