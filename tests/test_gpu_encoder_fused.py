"""The ResNet encoder's fused glue (scsfm_hip.encoder, csrc_enc/scsfm_encoder.hip) on the GPU against the ATen chain it
replaces: each op, forward and backward, at every stage shape of configs[1] (batch 12, 256 x 832) and at odd shapes,
then the whole ResnetEncoder.

The max-pool is exact: bit-identical to ATen, forward and backward.  BatchNorm sums in another order than MIOpen, so the
yardstick is the same chain evaluated in fp64 with the fp32 chain measured beside it (tests/_encoder_ref.py):
max|fused32 - ref64| <= 2 max|aten32 - ref64| + 4 u max|ref64| per tensor."""
import copy

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import _encoder_ref as R
from _util import report

pytestmark = pytest.mark.gpu

DEV = "cuda"


def bits(t):
    return t.contiguous().view(torch.int32)


def _fused(case, n_forward=1):
    from scsfm_hip import encoder as E
    C = case["x"].shape[1]
    bn = nn.BatchNorm2d(C, eps=R.EPS, momentum=R.MOMENTUM).to(DEV).train()
    with torch.no_grad():
        bn.weight.copy_(case["gamma"])
        bn.bias.copy_(case["beta"])
        bn.running_mean.copy_(case["running_mean"])
        bn.running_var.copy_(case["running_var"])
    x = case["x"].float().requires_grad_()
    identity = None if case["identity"] is None else case["identity"].float().requires_grad_()
    out = {}
    for k in range(n_forward):
        y = E.bn_act(x, bn, identity, relu=case["mode"] != 0)
        if k == 0:
            out["running_mean_1"], out["running_var_1"] = bn.running_mean.clone(), bn.running_var.clone()
    stat = y.grad_fn.saved_tensors[3]
    y.backward(case["g"].float())
    out.update(y=y.detach(), dx=x.grad, dgamma=bn.weight.grad, dbeta=bn.bias.grad, mean=stat[0], invstd=stat[1],
               running_mean=bn.running_mean.clone(), running_var=bn.running_var.clone(),
               num_batches_tracked=int(bn.num_batches_tracked))
    if identity is not None:
        out["d_identity"] = identity.grad
    return {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in out.items()}


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("shape", R.STAGE_SHAPES + R.ODD_SHAPES)
def test_bn_act_meets_the_contract(shape, mode):
    case = R.make_case(shape, mode, seed=sum(shape) + mode, device=DEV)
    fused = _fused(case)
    again = _fused(case)
    for k, v in fused.items():  # fixed summation order: the same bits from call to call
        assert v == again[k] if isinstance(v, int) else torch.equal(bits(v), bits(again[k])), k
    R.check_contract(f"gpu {R.MODES[mode]} {shape}", fused, R.aten_chain(case, torch.float32),
                     R.aten_chain(case, torch.float64))


@pytest.mark.parametrize("mode", [1, 2])
def test_three_forwards_of_one_module_before_one_backward(mode):
    case = R.make_case((12, 128, 32, 104), mode, seed=7, device=DEV)
    R.check_contract(f"gpu {R.MODES[mode]} x3", _fused(case, 3), R.aten_chain(case, torch.float32, 3),
                     R.aten_chain(case, torch.float64, 3))


def test_relu_mask_is_the_forwards():
    from scsfm_hip import encoder as E
    case = R.make_case((12, 64, 64, 208), 2, seed=2, device=DEV)
    out = _fused(case)
    want = torch.where(out["y"] > 0, case["g"].float().cpu(), torch.zeros(()))
    assert torch.equal(out["d_identity"], want)
    # a NaN passes the clamp (a diverged run still shows)
    bn = nn.BatchNorm2d(4).to(DEV).train()
    x = torch.randn(2, 4, 6, 8, device=DEV)
    ident = torch.zeros_like(x)
    ident[1, 2, 3, 4] = float("nan")
    y = E.bn_act(x, bn, ident)
    assert bool(torch.isnan(y[1, 2, 3, 4])) and int(torch.isnan(y).sum()) == 1


@pytest.mark.parametrize("shape", [(12, 64, 128, 416), (1, 3, 2, 2), (2, 5, 3, 3), (3, 2, 5, 263), (1, 4, 7, 131),
                                   (1, 1, 1, 1)])
def test_max_pool_is_bit_identical_to_aten(shape):
    from scsfm_hip import encoder as E
    x1 = R.pool_input(shape, seed=sum(shape), device=DEV).requires_grad_()
    x2 = x1.detach().clone().requires_grad_()
    out, ref = E.max_pool(x1), F.max_pool2d(x2, 3, 2, 1)
    assert out.shape == ref.shape and torch.equal(bits(out), bits(ref))
    g = torch.randn(ref.shape, device=DEV, generator=torch.Generator(device=DEV).manual_seed(1))
    out.backward(g)
    ref.backward(g)
    assert torch.equal(bits(x1.grad), bits(x2.grad))
    x3 = torch.randn(shape, device=DEV, generator=torch.Generator(device=DEV).manual_seed(2))  # (no ties, negatives)
    assert torch.equal(bits(E.max_pool(x3)), bits(F.max_pool2d(x3, 3, 2, 1)))


@pytest.fixture
def deterministic_miopen():
    old = torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = True, False
    yield
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = old


def _encoder_run(enc, xs, ws, reference):
    """features of every forward, parameter gradients of the seeded linear loss over all of them, buffers afterwards"""
    enc.zero_grad(set_to_none=True)
    feats = [(enc.forward_reference(x) if reference else enc(x)) for x in xs]
    sum((f * w).sum() for fs, wl in zip(feats, ws) for f, w in zip(fs, wl)).backward()
    out = {f"f{i}_{k}": f.detach() for k, fs in enumerate(feats) for i, f in enumerate(fs)}
    out.update({"grad " + n: p.grad for n, p in enc.named_parameters() if p.grad is not None})
    out.update({"buffer " + n: b.detach().clone() for n, b in enc.named_buffers() if b.is_floating_point()})
    counters = [int(b) for n, b in enc.named_buffers() if not b.is_floating_point()]
    return out, counters


@pytest.mark.parametrize("images,forwards", [(1, 1), (2, 1), (1, 3)])
def test_whole_encoder_against_the_fp64_chain(images, forwards, deterministic_miopen, monkeypatch):
    """The five feature maps, all parameter gradients and the running statistics: fused fp32 and reference fp32, each
    against the reference chain in fp64, the same inequality per tensor; with three forwards of the same net before one
    backward as train.py's compute_depth runs them.

    The seeded net is first moved off its kinks (tests/_encoder_ref.condition_encoder): a pre-activation within rounding
    of a ReLU's 0 makes any fp32 gradient of the whole net jump by 1e-3 of its scale, ATen's as well, which no bound on
    rounding covers; with every pre-activation and pooling gap at least KINK_MARGIN from it the comparison measures
    rounding only."""
    from models.resnet_encoder import ResnetEncoder
    from scsfm_hip import encoder as E
    torch.manual_seed(images)
    enc = ResnetEncoder(18, False, num_input_images=images).to(DEV).train()
    gen = torch.Generator(device=DEV).manual_seed(3)
    xs = [torch.randn(2, 3 * images, 64, 128, device=DEV, generator=gen) for _ in range(forwards)]
    enc64 = copy.deepcopy(enc).double()
    rounds, lo_v, lo_gap = R.condition_encoder(enc64, [x.double() for x in xs], seed=5 + images)
    assert min(lo_v, lo_gap) >= R.KINK_MARGIN
    enc.load_state_dict(enc64.state_dict())  # (fp32-representable values: an exact copy)
    assert all(torch.equal(a.double(), b) for a, b in zip(enc.state_dict().values(), enc64.state_dict().values()))
    report(f"gpu ResnetEncoder images={images} forwards={forwards}: off the kinks after {rounds} re-draws, smallest "
           f"|pre-activation| {lo_v:.2e}, smallest pooling gap {lo_gap:.2e}")
    start = copy.deepcopy(enc.state_dict())
    with torch.no_grad():
        shapes = [f.shape for f in enc.forward_reference(xs[0])]
    ws = [[torch.randn(s, device=DEV, generator=gen) / s.numel() ** 0.5 for s in shapes] for _ in range(forwards)]
    calls = []
    real = E.bn_act
    monkeypatch.setattr(E, "bn_act", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    enc.load_state_dict(start)
    fused, n_fused = _encoder_run(enc, xs, ws, reference=False)
    assert len(calls) == 20 * forwards, "the fused path was not taken by every BatchNorm"
    enc.load_state_dict(start)
    ref32, n_ref = _encoder_run(enc, xs, ws, reference=True)
    enc64.load_state_dict(start)
    ref64, _ = _encoder_run(enc64, [x.double() for x in xs], [[w.double() for w in wl] for wl in ws], reference=True)
    assert n_fused == n_ref == [forwards] * 20
    failures, worst = [], 0.0
    for name, r in ref64.items():
        ef = float((fused[name].double() - r).abs().max())
        ea = float((ref32[name].double() - r).abs().max())
        bound = 2 * ea + 4 * R.U * float(r.abs().max())
        worst = max(worst, ef / bound if bound else 0.0)
        if not ef <= bound:
            failures.append((name, ef, ea, bound))
    report(f"gpu ResnetEncoder images={images} forwards={forwards}: {len(ref64)} tensors, worst fused error "
           f"{worst:.3f} of its bound")
    for name in ("f4_0", "grad encoder.conv1.weight", "buffer encoder.bn1.running_var"):
        r = ref64[name]
        report(f"   {name}: max|fused32-ref64| {float((fused[name].double() - r).abs().max()):.3e}  max|aten32-ref64| "
               f"{float((ref32[name].double() - r).abs().max()):.3e}  scale {float(r.abs().max()):.3e}")
    assert not failures, failures
