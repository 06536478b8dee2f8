"""train.py --freeze-bn without a GPU: scsfm_hip.encoder_frozen.freeze holds every BatchNorm2d of a net in eval mode through
train() / eval() / train() without changing its state dict, its pickling or its parameters' names; with ``affine`` exactly
the BatchNorm parameters stop training; a frozen net in training mode on CPU is forward_reference's ATen chain bit for bit,
forward and backward, and writes no buffer; every condition of ``encoder_frozen.applies`` on its own (against a stand-in
that lets CPU tensors pass for device tensors); and the flag parses and is refused when a net has no statistics to hold."""
import copy
import io
import pickle

import pytest
import torch
import torch.nn as nn

import logger  # noqa: F401  (its writers keep the sys.stdout of their import: not the one of a test's capsys, which closes)


def _refuse(*a, **k):
    raise AssertionError("a fused path was taken")


def _bns(net):
    return [m for m in net.modules() if isinstance(m, nn.BatchNorm2d)]


def _seeded_statistics(net, seed=0):
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in _bns(net):
            m.running_mean.copy_(0.1 * torch.randn(m.num_features, generator=gen))
            m.running_var.copy_(0.5 + torch.rand(m.num_features, generator=gen))
            m.weight.copy_(1 + 0.1 * torch.randn(m.num_features, generator=gen))
            m.bias.copy_(0.1 * torch.randn(m.num_features, generator=gen))
            m.num_batches_tracked.fill_(7)


def _nets():
    import models
    from models.resnet_encoder import ResnetEncoder
    return {"ResnetEncoder(18)": (lambda: ResnetEncoder(18, False), 20), "ResnetEncoder(50)": (lambda: ResnetEncoder(50, False), 53),
            "DispResNet(18)": (lambda: models.DispResNet(18, False), 20), "PoseResNet(18)": (lambda: models.PoseResNet(18, False), 20)}


@pytest.mark.parametrize("name", ["ResnetEncoder(18)", "ResnetEncoder(50)", "DispResNet(18)", "PoseResNet(18)"])
def test_freeze_holds_every_batchnorm_and_nothing_else(name):
    from scsfm_hip import encoder_frozen as EF
    make, count = _nets()[name]
    torch.manual_seed(0)
    net = make()
    _seeded_statistics(net)
    state = {k: v.clone() for k, v in net.state_dict().items()}
    grads = {k: p.requires_grad for k, p in net.named_parameters()}
    assert EF.freeze(net) == count == len(_bns(net))
    assert all(EF.is_frozen(m) and isinstance(m, nn.BatchNorm2d) and not m.training for m in _bns(net))
    for mode in (net.train, net.eval, net.train):
        mode()
        assert not any(m.training for m in _bns(net))
    assert net.training and all(m.training for m in net.modules() if isinstance(m, nn.Conv2d))
    # the state dict: the same names in the same order, the same values; a reference-layout dict loads strictly
    assert list(net.state_dict()) == list(state) and all(torch.equal(state[k], v) for k, v in net.state_dict().items())
    assert grads == {k: p.requires_grad for k, p in net.named_parameters()}
    plain = make()
    plain.load_state_dict(net.state_dict(), strict=True)
    other = {k: torch.full_like(v, 3) for k, v in plain.state_dict().items()}
    net.load_state_dict(other, strict=True)
    assert all(torch.equal(other[k], v) for k, v in net.state_dict().items())
    assert not any(m.training for m in _bns(net))
    # copies stay frozen
    buf = io.BytesIO()
    torch.save(net, buf)
    buf.seek(0)
    for twin in (copy.deepcopy(net), pickle.loads(pickle.dumps(net)), torch.load(buf, weights_only=False)):
        assert len(_bns(twin)) == count and all(EF.is_frozen(m) and not m.training for m in _bns(twin.train()))
        assert all(torch.equal(a, b) for a, b in zip(net.state_dict().values(), twin.state_dict().values()))
    assert EF.freeze(net) == count  # (again: the same modules, still frozen)


@pytest.mark.parametrize("name", ["ResnetEncoder(18)", "DispResNet(18)"])
def test_affine_turns_off_exactly_the_batchnorm_parameters(name):
    from scsfm_hip import encoder_frozen as EF
    make, count = _nets()[name]
    net = make()
    before = {k: p.requires_grad for k, p in net.named_parameters()}
    bn_params = {f"{prefix}.{w}" for prefix, m in net.named_modules() if isinstance(m, nn.BatchNorm2d)
                 for w in ("weight", "bias")}
    assert len(bn_params) == 2 * count and all(before[k] for k in bn_params)
    assert EF.freeze(net, affine=True) == count
    after = {k: p.requires_grad for k, p in net.named_parameters()}
    assert {k for k in before if before[k] != after[k]} == bn_params and not any(after[k] for k in bn_params)


def test_freeze_refuses_what_it_cannot_hold():
    from scsfm_hip import encoder_frozen as EF
    with pytest.raises(ValueError):
        EF.freeze(nn.Sequential(nn.BatchNorm2d(4, track_running_stats=False)))

    class Odd(nn.BatchNorm2d):
        pass
    with pytest.raises(TypeError):
        EF.freeze(nn.Sequential(Odd(4)))
    assert EF.freeze(nn.Sequential(nn.Conv2d(3, 4, 1), nn.BatchNorm1d(4))) == 0


@pytest.mark.parametrize("layers", [18, 50])
def test_frozen_training_mode_on_cpu_is_the_reference_chain(layers, monkeypatch):
    from models.resnet_encoder import ResnetEncoder, _frozen_applies
    from scsfm_hip import encoder as E, encoder_eval as EE, encoder_frozen as EF
    for mod in (E, EE, EF):
        monkeypatch.setattr(mod, "bn_act", _refuse)
    for mod in (E, EE):
        monkeypatch.setattr(mod, "max_pool", _refuse)
    torch.manual_seed(0)
    enc = ResnetEncoder(layers, False)
    _seeded_statistics(enc)
    EF.freeze(enc)
    enc.train()
    x = torch.randn(2, 3, 32, 64)
    state = {k: v.clone() for k, v in enc.state_dict().items()}
    assert not _frozen_applies(enc.encoder.conv1(x), enc.encoder.bn1)
    params = [p for p in enc.parameters() if p.requires_grad]
    got = enc(x)
    g_got = torch.autograd.grad(sum(f.sum() for f in got), params)
    ref = enc.forward_reference(x)
    g_ref = torch.autograd.grad(sum(f.sum() for f in ref), params)
    assert len(got) == len(ref) == 5 and all(torch.equal(a, b) for a, b in zip(got, ref))
    assert all(torch.equal(a, b) for a, b in zip(g_got, g_ref))
    assert all(torch.equal(state[k], v) for k, v in enc.state_dict().items())  # no buffer (and no parameter) was written
    # ... and these are the eval-mode statistics: an unfrozen twin in eval mode gives the same features
    twin = ResnetEncoder(layers, False)
    twin.load_state_dict(state)
    with torch.no_grad():
        assert all(torch.equal(a, b) for a, b in zip(got, twin.eval().forward_reference(x)))


def _frozen_bn(n=4, **kw):
    from scsfm_hip import encoder_frozen as EF
    bn = nn.BatchNorm2d(n, **kw)
    EF.freeze(bn)
    return bn


def test_what_disqualifies_a_call(monkeypatch):
    """every condition of ``applies`` on its own: ``_plain`` is replaced by a stand-in without the device test, so that a
    CPU fp32 tensor through a frozen module with grad mode on qualifies and one change at a time disqualifies it"""
    from scsfm_hip import encoder_frozen as EF
    x = torch.randn(2, 4, 3, 3)
    assert not EF.applies(x, _frozen_bn()) and not EF.applies(x)   # a CPU tensor never qualifies
    with pytest.raises(ValueError):
        EF.bn_act(x, _frozen_bn())
    monkeypatch.setattr(EF, "_plain", lambda t: t.dtype == torch.float32 and t.is_contiguous())
    monkeypatch.delenv("SCSFM_FROZEN_TORCH", raising=False)
    assert EF.applies(x, _frozen_bn()) and EF.applies(x, _frozen_bn(), _frozen_bn()) and EF.applies(x)
    # the form without a ReLU is bn_act's to take but not the dispatch's (it measured slower than ATen's single kernel)
    assert EF.qualifies(x, _frozen_bn()) and not EF.applies(x, _frozen_bn(), relu=False)
    thawed = _frozen_bn()
    thawed.training = True
    bad_modules = {"not frozen, eval mode": nn.BatchNorm2d(4).eval(), "not frozen, training": nn.BatchNorm2d(4).train(),
                   "frozen, set to training by hand": thawed, "affine=False": _frozen_bn(affine=False),
                   "fp64 vectors": _frozen_bn().double(), "other width": _frozen_bn(5)}
    for why, bn in bad_modules.items():
        assert not EF.applies(x, bn) and not EF.applies(x, _frozen_bn(), bn) and not EF.qualifies(x, bn), why
        with pytest.raises(ValueError):
            EF.bn_act(x, bn)
    bad_inputs = {"fp64": x.double(), "channels_last": x.contiguous(memory_format=torch.channels_last), "3-D": x[0],
                  "empty": x[:0], "strided": x[:, :, ::2]}
    for why, t in bad_inputs.items():
        assert not EF.applies(t, _frozen_bn()) and not EF.applies(t) and not EF.qualifies(t, _frozen_bn()), why
        with pytest.raises(ValueError):
            EF.bn_act(t, _frozen_bn())
    with torch.no_grad():
        assert not EF.applies(x, _frozen_bn()) and not EF.applies(x)
        with pytest.raises(ValueError):
            EF.bn_act(x, _frozen_bn())
    monkeypatch.setenv("SCSFM_FROZEN_TORCH", "1")
    assert not EF.applies(x, _frozen_bn()) and not EF.applies(x)
    monkeypatch.setenv("SCSFM_FROZEN_TORCH", "0")
    assert EF.applies(x, _frozen_bn())
    with pytest.raises(ValueError):   # the residual form ends in a ReLU; the identity has x's shape
        EF.bn_act(x, _frozen_bn(), identity=x, relu=False)
    with pytest.raises(ValueError):
        EF.bn_act(x, _frozen_bn(), identity=x[:1])


def test_the_other_two_paths_keep_their_conditions():
    """a frozen module is an eval-mode module to them: the training path refuses it, the eval path takes it under no_grad
    only (its own conditions are tests/test_encoder_eval_dispatch.py's)"""
    from scsfm_hip import encoder as E, encoder_eval as EE
    x = torch.randn(2, 4, 3, 3)
    assert not E.applies(x, _frozen_bn()) and not EE.applies(x, _frozen_bn())
    import inspect
    from models import resnet_encoder as RE
    src = inspect.getsource(RE._bn_act)
    assert src.index("_fused_applies") < src.index("_frozen_applies") < src.index("_eval_applies")
    assert "relu=act is not None" in src


def test_the_flag_parses_and_needs_statistics(capsys):
    import train
    base = ["/tmp/x", "--name", "n"]
    assert train.parser.parse_args(base).freeze_bn == "off"
    for mode in ("off", "stats", "all"):
        assert train.parser.parse_args(base + ["--freeze-bn", mode]).freeze_bn == mode
    with pytest.raises(SystemExit):
        train.parser.parse_args(base + ["--freeze-bn", "some"])
    capsys.readouterr()
    parse = lambda *extra: train.parser.parse_args(base + list(extra))  # noqa: E731
    lacking = lambda *extra: [n for n, _ in train.nets_without_statistics(parse(*extra))]  # noqa: E731
    assert lacking("--with-pretrain", "0") == [] and lacking("--freeze-bn", "stats") == []   # off; ImageNet weights
    assert lacking("--freeze-bn", "stats", "--with-pretrain", "0") == ["DispResNet", "PoseResNet"]
    assert lacking("--freeze-bn", "all", "--with-pretrain", "0", "--pretrained-disp", "d.tar") == ["PoseResNet"]
    assert lacking("--freeze-bn", "all", "--with-pretrain", "0", "--pretrained-pose", "p.tar") == ["DispResNet"]
    assert lacking("--freeze-bn", "stats", "--with-pretrain", "0", "--pretrained-disp", "d", "--pretrained-pose", "p") == []


@pytest.mark.parametrize("extra,named,spared", [
    ((), ("DispResNet", "PoseResNet"), ()),
    (("--pretrained-disp", "/nonexistent/d.tar"), ("PoseResNet",), ("DispResNet",)),
    (("--pretrained-pose", "/nonexistent/p.tar"), ("DispResNet",), ("PoseResNet",))])
def test_main_refuses_the_flag_at_argument_parsing(extra, named, spared, monkeypatch, capsys):
    """parser.error (exit status 2, the net named) before any dataset, device or checkpoint is touched: the data
    directory and the checkpoints do not exist"""
    import train
    monkeypatch.setattr("sys.argv", ["train.py", "/nonexistent/data", "--name", "n", "--with-pretrain", "0", "--freeze-bn",
                                     "stats", *extra])
    monkeypatch.setattr(train, "build_datasets", _refuse)
    with pytest.raises(SystemExit) as e:
        train.main()
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert "--freeze-bn stats" in err and all(n in err for n in named) and not any(n in err for n in spared)
