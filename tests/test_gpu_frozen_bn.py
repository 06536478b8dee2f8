"""Frozen-statistics BatchNorm (scsfm_hip.encoder_frozen, csrc_fbn/scsfm_frozen_bn.hip) on the GPU against the ATen chain it
replaces -- nn.BatchNorm2d(...).eval() -> + identity -> relu, with grad: each mode's backward at the host simulator's
shapes, the stem's plane and past the grid's cap; the forward bit for bit scsfm_hip.encoder_eval's; what the node saves;
then the whole frozen ResnetEncoder(18) in training mode against the fp64 chain, ResNet-50's dispatch and one of its
Bottlenecks, and SCSFM_FROZEN_TORCH=1.  The yardstick is tests/_frozen_bn_ref.py's:
max|fused32 - ref64| <= 2 max|aten32 - ref64| + 4 u max|ref64| per tensor."""
import copy

import pytest
import torch
import torch.nn as nn

import _encoder_ref as ER
import _frozen_bn_ref as R
from _util import report

pytestmark = pytest.mark.gpu

DEV = "cuda"
PAST_THE_CAP = (5, 6560, 2, 2)   # 32800 planes of one task each: more tasks than the largest grid has waves


def bits(t):
    return t.contiguous().view(torch.int32)


def _frozen_module(case, affine=False):
    from scsfm_hip import encoder_frozen as EF
    bn = R.EV.eval_bn(case, torch.float32, DEV).train()
    assert EF.freeze(bn, affine=affine) == 1 and not bn.training
    return bn


def _fused(case, affine=False):
    from scsfm_hip import encoder_frozen as EF
    bn = _frozen_module(case, affine)
    buffers = [b.clone() for b in bn.buffers()]
    x = case["x"].float().requires_grad_()
    identity = None if case["identity"] is None else case["identity"].float().requires_grad_()
    y = EF.bn_act(x, bn, identity, relu=case["mode"] != 0)
    saved = [t.data_ptr() for t in y.grad_fn.saved_tensors]
    y.backward(case["g"].float())
    assert all(torch.equal(a, b) for a, b in zip(buffers, bn.buffers())), "a buffer was written"
    out = dict(y=y.detach(), dx=x.grad)
    if identity is not None:
        out["d_identity"] = identity.grad
    if not affine:
        out.update(dgamma=bn.weight.grad, dbeta=bn.bias.grad)
    else:
        assert bn.weight.grad is None and bn.bias.grad is None
    return {k: v.cpu() for k, v in out.items()}, (x.data_ptr() in saved, y.data_ptr() in saved, len(saved))


def test_the_cases_are_what_they_claim():
    n, waves, vec = R.tasks(PAST_THE_CAP)
    assert vec and n == 5 * 6560 > waves and waves == R.kernel_constants()[3] * 4
    assert R.tasks(R.STEM_PLANE)[0] > 64 * 50


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("shape", R.SHAPES + [R.STEM_PLANE, PAST_THE_CAP])
def test_backward_meets_the_contract(shape, mode):
    case = R.make_case(shape, mode, seed=sum(shape) + mode, device=DEV)
    fused, (saved_x, saved_y, n_saved) = _fused(case)
    again, _ = _fused(case)
    for k, v in fused.items():   # a fixed order of summation: the same bits from call to call
        assert torch.equal(bits(v), bits(again[k])), k
    assert saved_x and saved_y == (mode != 0) and n_saved == 1 + (mode != 0)
    ref32, ref64 = R.aten_chain(case, torch.float32), R.aten_chain(case, torch.float64)
    R.check_frozen_contract(f"gpu frozen {R.MODES[mode]} {shape}", fused, ref32, ref64)
    # without parameter gradients: x is not kept, dx and d_identity carry the same bits
    bare, (saved_x, saved_y, n_saved) = _fused(case, affine=True)
    assert not saved_x and saved_y == (mode != 0) and n_saved == int(mode != 0)
    assert set(bare) == set(fused) - {"dgamma", "dbeta"} and all(torch.equal(bits(bare[k]), bits(fused[k])) for k in bare)


@pytest.mark.parametrize("mode", [1, 2])
def test_planted_nan_and_inf_are_atens(mode):
    shape = (2, 3, 4, 8)
    case = R.make_case(shape, mode, seed=sum(shape) + mode, device=DEV, special=True)
    fused, _ = _fused(case)
    assert bool(torch.isnan(fused["y"][0, 0, 0, 0])) and float(fused["dx"][0, 0, 0, 0]) != 0   # the gradient passes a NaN
    R.check_frozen_contract(f"gpu frozen {R.MODES[mode]} {shape} nan_inf", fused, R.aten_chain(case, torch.float32),
                            R.aten_chain(case, torch.float64))


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("shape", [(3, 2, 5, 263), (2, 512, 8, 26), R.STEM_PLANE])
def test_forward_is_the_eval_kernels_bit_for_bit(shape, mode):
    from scsfm_hip import encoder_eval as EE, encoder_frozen as EF
    case = R.make_case(shape, mode, seed=sum(shape) + mode, device=DEV)
    bn = _frozen_module(case)
    x = case["x"].float()
    identity = None if case["identity"] is None else case["identity"].float()
    y = EF.bn_act(x, bn, identity, relu=mode != 0)
    assert y.requires_grad and type(y.grad_fn).__name__.startswith("_FrozenBnAct")
    with torch.no_grad():
        assert not EF.applies(x, bn) and not EF.qualifies(x, bn) and EE.applies(x, bn)
        want = EE.bn_act(x, bn, identity, relu=mode != 0)
    assert torch.equal(bits(y.detach()), bits(want))


def test_a_merely_eval_mode_module_is_refused():
    from scsfm_hip import encoder_frozen as EF
    x = torch.randn(2, 4, 6, 8, device=DEV)
    bn = nn.BatchNorm2d(4).to(DEV).eval()
    assert not EF.applies(x, bn) and not EF.qualifies(x, bn)
    with pytest.raises(ValueError):
        EF.bn_act(x, bn)
    EF.freeze(bn)
    assert EF.qualifies(x, bn) and not EF.applies(x, bn, relu=False)
    assert EF.applies(x, bn) and not EF.applies(x.double(), bn) and not EF.applies(x[:, :, ::2], bn)
    assert not EF.applies(x.contiguous(memory_format=torch.channels_last), bn)


@pytest.fixture
def deterministic_miopen():
    old = torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = True, False
    yield
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = old


def _net_run(net, x, ws, reference):
    """outputs, the gradient with respect to the input and to every parameter that trains, of a seeded linear loss"""
    net.zero_grad(set_to_none=True)
    x = x.detach().clone().requires_grad_()
    outs = net.forward_reference(x) if reference else net(x)
    outs = outs if isinstance(outs, (list, tuple)) else [outs]
    sum((o * w).sum() for o, w in zip(outs, ws)).backward()
    out = {f"out_{i}": o.detach() for i, o in enumerate(outs)}
    out["grad x"] = x.grad
    out.update({"grad " + n: p.grad for n, p in net.named_parameters() if p.grad is not None})
    return out


def _count_calls(monkeypatch):
    """-> the list every call of the three fused bn_act's and of ATen's batch_norm is named in.  A frozen net in training
    mode sends every BatchNorm with a ReLU behind it through encoder_frozen and the down-sample branches' (three in
    ResNet-18, four in ResNet-50; no ReLU, nothing to fuse, measured slower: encoder_frozen.applies) through ATen."""
    import torch.nn.functional as F
    from scsfm_hip import encoder as E, encoder_eval as EE, encoder_frozen as EF
    calls = []

    def counted(name, real):
        return lambda *a, **k: (calls.append(name), real(*a, **k))[1]
    for name, mod in (("encoder", E), ("encoder_eval", EE), ("encoder_frozen", EF)):
        monkeypatch.setattr(mod, "bn_act", counted(name, mod.bn_act))
    monkeypatch.setattr(F, "batch_norm", counted("aten", F.batch_norm))
    return calls


def _check_tensors(what, fused, ref32, ref64):
    assert set(fused) == set(ref32) == set(ref64), set(fused) ^ set(ref64)
    failures, worst = [], (0.0, "")
    for name, r in ref64.items():
        assert bool(torch.isfinite(fused[name]).all()), (what, name)
        ef = float((fused[name].double() - r).abs().max())
        ea = float((ref32[name].double() - r).abs().max())
        bound = 2 * ea + 4 * R.U * float(r.abs().max())
        worst = max(worst, (ef / bound if bound else 0.0, name))
        if not ef <= bound:
            failures.append((name, ef, ea, bound))
    report(f"{what}: {len(ref64)} tensors, worst fused error {worst[0]:.3f} of its bound ({worst[1]})")
    assert not failures, (what, failures)


@pytest.mark.parametrize("affine", [False, True], ids=["stats", "all"])
def test_whole_frozen_encoder_against_the_fp64_chain(affine, deterministic_miopen, monkeypatch):
    """ResnetEncoder(18), frozen, in training mode, batch 2 at 64 x 96: the five feature maps, the input gradient and
    every parameter gradient of the fused path and of the ATen chain through the same frozen modules in fp32, each
    against that chain in fp64; 17 calls through encoder_frozen, the three down-sample branches' through ATen's batch_norm
    (encoder_frozen.applies routes the form without a ReLU there) and none through the training-mode op; 20 through
    encoder_eval once eval() + no_grad is entered; no buffer written.  The net is moved off its
    kinks first (tests/_encoder_ref.condition_encoder over the eval-statistics sites).  The ATen chain's own fp32
    pre-activation error e is measured on the device, and KINK_MARGIN has to be 5 e: a fused forward that keeps the
    contract is within 2 e of the fp64 chain (plus the floor), the ATen chain within e, so a mask can differ between
    any two of the three evaluations only where a pre-activation is below 3 e."""
    from models.resnet_encoder import ResnetEncoder
    from scsfm_hip import encoder_frozen as EF
    torch.manual_seed(18)
    enc = ResnetEncoder(18, False)
    R.randomise_bn(enc, 18)
    x = torch.randn(2, 3, 64, 96, generator=torch.Generator().manual_seed(3)).to(DEV)
    enc = enc.to(DEV)
    assert EF.freeze(enc, affine=affine) == 20
    enc.train()
    enc64 = copy.deepcopy(enc).double()
    rounds, lo_v, lo_gap = ER.condition_encoder(enc64, [x.double()], seed=6, sites=R.eval_relu_sites)
    assert min(lo_v, lo_gap) >= ER.KINK_MARGIN
    enc.load_state_dict(enc64.state_dict())  # (fp32-representable values: an exact copy)
    assert all(torch.equal(a.double(), b) for a, b in zip(enc.state_dict().values(), enc64.state_dict().values()))
    err = ER.preactivation_error(enc, enc64, [x], R.eval_relu_sites)
    what = f"gpu frozen ResnetEncoder(18) {'all' if affine else 'stats'}"
    report(f"{what}: off the kinks after {rounds} re-draws, smallest |pre-activation| {lo_v:.2e}, smallest pooling gap "
           f"{lo_gap:.2e}; fp32 pre-activation error of the ATen chain {err:.2e}")
    assert ER.KINK_MARGIN >= 5 * err
    buffers = {n: b.clone() for n, b in enc.named_buffers()}
    gen = torch.Generator(device=DEV).manual_seed(9)
    with torch.no_grad():
        shapes = [f.shape for f in enc.forward_reference(x)]
    ws = [torch.randn(s, device=DEV, generator=gen) / s.numel() ** 0.5 for s in shapes]
    calls = _count_calls(monkeypatch)
    fused = _net_run(enc, x, ws, reference=False)
    assert sorted(calls) == ["aten"] * 3 + ["encoder_frozen"] * 17, calls
    del calls[:]
    ref32 = _net_run(enc, x, ws, reference=True)
    assert calls == ["aten"] * 20, calls
    ref64 = _net_run(enc64, x.double(), [w.double() for w in ws], reference=True)
    del calls[:]
    enc.eval()
    with torch.no_grad():
        inference = enc(x)
    assert calls == ["encoder_eval"] * 20, calls
    # training sees inference's values bit for bit up to the first down-sample branch (layer2's), which ATen rounds its way
    assert all(torch.equal(bits(inference[i]), bits(fused[f"out_{i}"])) for i in (0, 1))
    assert not any(m.training for m in enc.train().modules() if isinstance(m, nn.BatchNorm2d))
    n_bn_grads = sum(1 for n in fused if n.startswith("grad ") and (".bn" in n or "downsample.1" in n))
    assert n_bn_grads == (0 if affine else 40) and len(fused) == 5 + 1 + 20 + n_bn_grads
    _check_tensors(what, fused, ref32, ref64)
    assert all(torch.equal(b, buffers[n]) for n, b in enc.named_buffers()) and len(buffers) == 60


def test_frozen_torch_sends_the_frozen_net_down_aten(deterministic_miopen, monkeypatch):
    from models.resnet_encoder import ResnetEncoder
    from scsfm_hip import encoder_frozen as EF
    torch.manual_seed(19)
    enc = ResnetEncoder(18, False)
    R.randomise_bn(enc, 19)
    enc = enc.to(DEV)
    EF.freeze(enc)
    enc.train()
    x = torch.randn(2, 3, 64, 96, device=DEV)
    ws = [torch.ones(()).to(DEV)] * 5
    monkeypatch.setenv("SCSFM_FROZEN_TORCH", "1")
    calls = _count_calls(monkeypatch)
    got = _net_run(enc, x, ws, reference=False)
    assert calls == ["aten"] * 20, calls
    ref = _net_run(enc, x, ws, reference=True)
    assert set(got) == set(ref) and all(torch.equal(bits(got[k]), bits(ref[k])) for k in ref)
    monkeypatch.setenv("SCSFM_FROZEN_TORCH", "0")
    del calls[:]
    _net_run(enc, x, ws, reference=False)
    assert sorted(calls) == ["aten"] * 3 + ["encoder_frozen"] * 17, calls


def test_frozen_resnet50_takes_the_fused_path(deterministic_miopen, monkeypatch):
    """Dispatch and finiteness only, for the reason tests/test_gpu_encoder_fused.py's
    test_resnet50_encoder_takes_the_fused_path gives (at this depth two fp32 evaluations cut different entries at the deep
    ReLUs); the values are held to the contract on one Bottleneck below."""
    from models.resnet_encoder import ResnetEncoder
    from scsfm_hip import encoder_frozen as EF
    torch.manual_seed(51)
    enc = ResnetEncoder(50, False)
    R.randomise_bn(enc, 51)
    enc = enc.to(DEV)
    assert EF.freeze(enc) == 53
    enc.train()
    buffers = [b.clone() for b in enc.buffers()]
    x = torch.randn(2, 3, 64, 128, device=DEV, generator=torch.Generator(device=DEV).manual_seed(4))
    with torch.no_grad():
        shapes = [f.shape for f in enc.forward_reference(x)]
    assert [s[1] for s in shapes] == [64, 256, 512, 1024, 2048]
    ws = [torch.randn(s, device=DEV) / s.numel() ** 0.5 for s in shapes]
    calls = _count_calls(monkeypatch)
    fused = _net_run(enc, x, ws, reference=False)
    assert sorted(calls) == ["aten"] * 4 + ["encoder_frozen"] * 49, calls
    params = [n for n, p in enc.named_parameters() if not n.startswith("encoder.fc.")]
    assert len(params) == 53 * 3 and all("grad " + n in fused for n in params)
    for name, t in fused.items():
        assert bool(torch.isfinite(t).all()), name
        if name.startswith("grad "):
            assert float(t.abs().max()) > 0, name
    assert all(torch.equal(a, b) for a, b in zip(buffers, enc.buffers()))


def test_frozen_bottleneck_with_a_downsample_branch_against_the_fp64_chain(deterministic_miopen, monkeypatch):
    """layer2[0] of ResNet-50 (stride 2; three BatchNorms through encoder_frozen, the down-sample branch's through ATen) at
    2 x 256 x 16 x 24"""
    from models.resnet_encoder import ResnetEncoder
    from scsfm_hip import encoder_frozen as EF
    torch.manual_seed(50)
    enc = ResnetEncoder(50, False)
    R.randomise_bn(enc, 50)
    block = copy.deepcopy(enc.encoder.layer2[0]).to(DEV)
    assert type(block).__name__ == "Bottleneck" and block.downsample is not None and EF.freeze(block) == 4
    block.train()
    x = torch.relu(torch.randn(2, 256, 16, 24, generator=torch.Generator().manual_seed(4))).to(DEV)
    block64 = copy.deepcopy(block).double()
    rounds, lo_v, _ = ER.condition_encoder(block64, [x.double()], seed=7, sites=R.eval_block_sites)
    assert lo_v >= ER.KINK_MARGIN
    block.load_state_dict(block64.state_dict())
    err = ER.preactivation_error(block, block64, [x], R.eval_block_sites)
    what = "gpu frozen Bottleneck layer2[0]"
    report(f"{what}: off the kinks after {rounds} re-draws, smallest |pre-activation| {lo_v:.2e}; fp32 pre-activation "
           f"error of the ATen chain {err:.2e}")
    assert ER.KINK_MARGIN >= 5 * err
    buffers = [b.clone() for b in block.buffers()]
    with torch.no_grad():
        shape = block.forward_reference(x).shape
    ws = [torch.randn(shape, device=DEV, generator=torch.Generator(device=DEV).manual_seed(2)) / shape.numel() ** 0.5]
    calls = _count_calls(monkeypatch)
    fused = _net_run(block, x, ws, reference=False)
    assert sorted(calls) == ["aten"] + ["encoder_frozen"] * 3, calls
    ref32 = _net_run(block, x, ws, reference=True)
    ref64 = _net_run(block64, x.double(), [w.double() for w in ws], reference=True)
    assert len(ref64) == 2 + 4 * 3
    _check_tensors(what, fused, ref32, ref64)
    assert all(torch.equal(a, b) for a, b in zip(buffers, block.buffers()))
