"""The fused stem (scsfm_hip.encoder.bn_act(..., pool=True), csrc_stem/scsfm_stem.hip) on the GPU: the forward bit for
bit the unfused pair E.max_pool(E.bn_act(x, bn)), the backward against that pair (dgamma / dbeta within one ulp, dx
within tests/_stem_ref.dx_bound) with and without a gradient on f0, and against the ATen chain in fp64 under the contract
of tests/_encoder_ref.py on inputs kept off the ReLU's and the pooling's kinks."""
import pytest
import torch
import torch.nn as nn

import _encoder_ref as R
import _stem_ref as SR

pytestmark = pytest.mark.gpu

DEV = "cuda"


def bits(t):
    return t.contiguous().view(torch.int32)


def _module(case):
    C = case["x"].shape[1]
    bn = nn.BatchNorm2d(C, eps=R.EPS, momentum=R.MOMENTUM).to(DEV).train()
    with torch.no_grad():
        bn.weight.copy_(case["gamma"])
        bn.bias.copy_(case["beta"])
        bn.running_mean.copy_(case["running_mean"])
        bn.running_var.copy_(case["running_var"])
    return bn


def _run(case, fused, with_f0=True, x=None, n_forward=1, zero_f0=False):
    """forward(s) and one backward through the fused stem or the unfused pair -> dict of device tensors"""
    from scsfm_hip import encoder as E
    bn = _module(case)
    x = (case["x"].float() if x is None else x.clone()).requires_grad_()
    out = {}
    for k in range(n_forward):
        if fused:
            f0, pooled = E.bn_act(x, bn, pool=True)
        else:
            f0 = E.bn_act(x, bn)
            pooled = E.max_pool(f0)
        if k == 0:
            out["running_mean_1"], out["running_var_1"] = bn.running_mean.clone(), bn.running_var.clone()
    node = f0.grad_fn if fused else pooled.grad_fn
    out["arg"] = node.saved_tensors[4] if fused else node.saved_tensors[0]
    out["stat"] = (f0.grad_fn if not fused else node).saved_tensors[3]
    if not fused:
        f0.retain_grad()
    grads = [case["g_pool"].float()]
    outs = [pooled]
    if with_f0:
        outs.append(f0)
        grads.append(torch.zeros_like(f0) if zero_f0 else case["g"].float())
    torch.autograd.backward(outs, grads)
    out.update(f0=f0.detach(), pooled=pooled.detach(), dx=x.grad, dgamma=bn.weight.grad, dbeta=bn.bias.grad,
               running_mean=bn.running_mean.clone(), running_var=bn.running_var.clone(),
               num_batches_tracked=bn.num_batches_tracked.clone())
    if not fused:
        out["t"] = f0.grad  # the pooling's gradient plus the one handed to f0
    return out


FORWARD_KEYS = ("f0", "pooled", "arg", "stat", "running_mean", "running_var", "num_batches_tracked")


def _assert_same_forward(a, b, what):
    for k in FORWARD_KEYS:
        x, y = a[k], b[k]
        if x.dtype == torch.float32:
            x, y = bits(x), bits(y)
        assert x.shape == y.shape and torch.equal(x, y), (what, k)


@pytest.mark.parametrize("shape", SR.SMALL_SHAPES + [SR.STEM_SHAPE])
def test_forward_and_backward_against_the_unfused_pair(shape):
    case = SR.make_case(shape, seed=sum(shape), device=DEV)
    pair, stem = _run(case, False), _run(case, True)
    _assert_same_forward(stem, pair, shape)
    again = _run(case, True)
    _assert_same_forward(stem, again, (shape, "second call"))
    for k in ("dx", "dgamma", "dbeta"):
        assert torch.equal(bits(stem[k]), bits(again[k])), (shape, k, "second call")
    if shape[1] > 2:  # the gamma = beta = 0 channel: all-zero windows, the first entry of the clipped window wins
        arg = stem["arg"][:, -1]
        PH, PW = arg.shape[1:]
        want = 3 * (torch.arange(PH, device=DEV) == 0)[:, None] + (torch.arange(PW, device=DEV) == 0)[None, :]
        assert torch.equal(arg.long(), want.expand(arg.shape).long()) and not bool(stem["pooled"][:, -1].any())

    def aux_of(p):
        stat = p["stat"]
        xhat = (case["x"].float() - stat[0].view(1, -1, 1, 1) - stat[2].view(1, -1, 1, 1)) * stat[1].view(1, -1, 1, 1)
        gprime = torch.where((p["f0"] > 0) | torch.isnan(p["f0"]), p["t"], torch.zeros((), device=DEV))
        return dict(gprime=gprime, xhat=xhat, gamma=case["gamma"].float(), invstd=stat[1])

    SR.check_backward_against_pair(f"gpu stem {shape} with f0 gradient", stem, pair, aux_of(pair))
    pair_n, stem_n = _run(case, False, with_f0=False), _run(case, True, with_f0=False)
    SR.check_backward_against_pair(f"gpu stem {shape} without f0 gradient", stem_n, pair_n, aux_of(pair_n))
    stem_z = _run(case, True, zero_f0=True)  # an absent gradient of f0 is an all-zero one
    for k in ("dx", "dgamma", "dbeta"):
        assert torch.equal(stem_n[k], stem_z[k]), (shape, k)


@pytest.mark.parametrize("shape", [(2, 4, 8, 16), (2, 5, 3, 3)])
def test_one_nan_in_x(shape):
    case = SR.make_case(shape, seed=3, device=DEV)
    x = case["x"].float()
    x[-1, 1, shape[2] // 2, shape[3] // 2] = float("nan")
    pair, stem = _run(case, False, x=x), _run(case, True, x=x)
    _assert_same_forward(stem, pair, (shape, "nan"))
    assert bool(torch.isnan(stem["pooled"][:, 1]).all()) and not bool(torch.isnan(stem["pooled"][:, 0]).any())


def _for_contract(out):
    keep = ("running_mean_1", "running_var_1", "f0", "pooled", "dx", "dgamma", "dbeta", "running_mean", "running_var")
    res = {k: out[k].cpu() for k in keep}
    res.update(mean=out["stat"][0].cpu(), invstd=out["stat"][1].cpu(),
               num_batches_tracked=int(out["num_batches_tracked"]))
    return res


@pytest.mark.parametrize("shape", SR.SMALL_SHAPES)
def test_backward_against_aten(shape):
    case = SR.make_conditioned_case(shape, seed=sum(shape) + 2, device=DEV)
    assert SR.off_the_kinks(case)
    R.check_contract(f"gpu stem {shape}", _for_contract(_run(case, True)), SR.aten_chain(case, torch.float32),
                     SR.aten_chain(case, torch.float64))


def test_three_forwards_of_one_module_before_one_backward():
    case = SR.make_conditioned_case((2, 4, 8, 16), seed=11, device=DEV)
    R.check_contract("gpu stem x3", _for_contract(_run(case, True, n_forward=3)),
                     SR.aten_chain(case, torch.float32, 3), SR.aten_chain(case, torch.float64, 3))


def test_only_the_pooled_gradient_missing():
    """(cannot happen in the nets) a gradient on f0 alone is the backward of relu(bn(x))"""
    from scsfm_hip import encoder as E
    case = SR.make_case((2, 4, 8, 16), seed=5, device=DEV)
    bn_a, bn_b = _module(case), _module(case)
    xa, xb = case["x"].float().requires_grad_(), case["x"].float().requires_grad_()
    f0, _ = E.bn_act(xa, bn_a, pool=True)
    f0.backward(case["g"].float())
    E.bn_act(xb, bn_b).backward(case["g"].float())
    assert torch.equal(xa.grad, xb.grad) and torch.equal(bn_a.weight.grad, bn_b.weight.grad)
    with pytest.raises(ValueError):
        E.bn_act(xa, bn_a, relu=False, pool=True)
    with pytest.raises(ValueError):
        E.bn_act(xa, bn_a, xb, pool=True)


def test_the_encoder_takes_the_fused_stem(monkeypatch):
    from models.resnet_encoder import ResnetEncoder
    from scsfm_hip import encoder as E

    def refuse(*a, **k):
        raise AssertionError("encoder.max_pool was called on the fused path")

    monkeypatch.setattr(E, "max_pool", refuse)
    torch.manual_seed(0)
    enc = ResnetEncoder(18, False).to(DEV).train()
    feats = enc(torch.randn(2, 3, 32, 64, device=DEV))
    assert len(feats) == 5 and feats[0].shape == (2, 64, 16, 32) and type(feats[0].grad_fn).__name__.startswith(
        "_BnReluPool")
    sum(f.sum() for f in feats[1:]).backward()  # f0 unread, as in the pose encoder
    assert enc.encoder.conv1.weight.grad is not None and bool(torch.isfinite(enc.encoder.conv1.weight.grad).all())
