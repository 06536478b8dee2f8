"""Which path the ResNet encoder takes in eval mode without a GPU: scsfm_hip.encoder_eval refuses CPU tensors, grad mode,
training-mode modules, modules without affine parameters or running statistics, fp64 and channels_last (each condition
also on its own, against a stand-in that lets CPU tensors pass for device tensors); eval-mode encoders on CPU run the ATen
chain (forward_reference) bit for bit; and scsfm_hip.encoder still refuses eval-mode modules."""
import pytest
import torch
import torch.nn as nn


def _refuse(*a, **k):
    raise AssertionError("the fused path was taken")


def _eval_bn(**kw):
    return nn.BatchNorm2d(4, **kw).eval()


def test_cpu_tensors_never_qualify():
    from scsfm_hip import encoder_eval as EE
    x = torch.randn(2, 4, 3, 3)
    with torch.no_grad():
        assert not EE.applies(x, _eval_bn()) and not EE.applies(x) and not EE.pool_applies(x)
        with pytest.raises(ValueError):
            EE.bn_act(x, _eval_bn())
        with pytest.raises(ValueError):
            EE.bn_act(x, _eval_bn(), pool=True)
        with pytest.raises(ValueError):
            EE.max_pool(x)


def test_what_disqualifies_a_call(monkeypatch):
    """every condition of ``applies`` on its own: ``_plain`` is replaced by a stand-in without the device test, so that a
    CPU fp32 tensor through an eval-mode module under no_grad qualifies and one change at a time disqualifies it"""
    from scsfm_hip import encoder_eval as EE
    monkeypatch.setattr(EE, "_plain", lambda t: t.dtype == torch.float32 and t.is_contiguous())
    monkeypatch.delenv("SCSFM_EVAL_TORCH", raising=False)
    x = torch.randn(2, 4, 3, 3)
    with torch.no_grad():
        assert EE.applies(x, _eval_bn()) and EE.applies(x, _eval_bn(), _eval_bn()) and EE.pool_applies(x)
        bad_modules = {"training": nn.BatchNorm2d(4).train(), "affine=False": _eval_bn(affine=False),
                       "track_running_stats=False": _eval_bn(track_running_stats=False),
                       "fp64 vectors": _eval_bn().double(), "other width": nn.BatchNorm2d(5).eval()}
        for why, bn in bad_modules.items():
            assert not EE.applies(x, bn) and not EE.applies(x, _eval_bn(), bn), why
            with pytest.raises(ValueError):
                EE.bn_act(x, bn)
        bad_inputs = {"fp64": x.double(), "channels_last": x.contiguous(memory_format=torch.channels_last),
                      "3-D": x[0], "empty": x[:0], "strided": x[:, :, ::2]}
        for why, t in bad_inputs.items():
            assert not EE.applies(t, _eval_bn()) and not EE.pool_applies(t), why
            with pytest.raises(ValueError):
                EE.bn_act(t, _eval_bn())
            with pytest.raises(ValueError):
                EE.max_pool(t)
        monkeypatch.setenv("SCSFM_EVAL_TORCH", "1")
        assert not EE.applies(x, _eval_bn()) and not EE.pool_applies(x)
        monkeypatch.setenv("SCSFM_EVAL_TORCH", "0")
        assert EE.applies(x, _eval_bn()) and EE.pool_applies(x)
    with torch.enable_grad():
        assert not EE.applies(x, _eval_bn()) and not EE.pool_applies(x)
        with pytest.raises(ValueError):
            EE.bn_act(x, _eval_bn())
        with pytest.raises(ValueError):
            EE.max_pool(x)


def test_the_training_path_still_refuses_eval_modules():
    from scsfm_hip import encoder as E
    x = torch.randn(2, 4, 3, 3)
    assert not E.applies(x, _eval_bn())
    with pytest.raises(ValueError):
        E.bn_act(x, _eval_bn())
    import inspect
    assert "bn.training" in inspect.getsource(E.applies)


@pytest.mark.parametrize("grad", [False, True], ids=["no_grad", "grad"])
@pytest.mark.parametrize("layers", [18, 50])
def test_eval_mode_on_cpu_is_the_reference_chain(layers, grad, monkeypatch):
    from models.resnet_encoder import ResnetEncoder, _eval_applies
    from scsfm_hip import encoder as E, encoder_eval as EE
    for mod in (E, EE):
        monkeypatch.setattr(mod, "bn_act", _refuse)
        monkeypatch.setattr(mod, "max_pool", _refuse)
    torch.manual_seed(0)
    enc = ResnetEncoder(layers, False).eval()
    with torch.no_grad():   # running statistics that are not the initial 0 / 1
        for m in enc.modules():
            if isinstance(m, nn.BatchNorm2d):
                m.running_mean.normal_(0, 0.1)
                m.running_var.uniform_(0.5, 1.5)
    x = torch.randn(2, 3, 32, 64)
    state = {k: v.clone() for k, v in enc.state_dict().items()}
    with torch.set_grad_enabled(grad):
        assert not _eval_applies(enc.encoder.conv1(x), enc.encoder.bn1)
        got = enc(x)
        ref = enc.forward_reference(x)
    assert len(got) == len(ref) == 5 and all(torch.equal(a, b) for a, b in zip(got, ref))
    assert all(torch.equal(state[k], v) for k, v in enc.state_dict().items())  # eval mode writes no buffer
