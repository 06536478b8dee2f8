"""The eval-mode encoder kernels (csrc_enceval/) on the host simulator against torch-CPU: BatchNorm from the running
statistics [+ residual] [+ ReLU], the stem's BatchNorm / ReLU fused with its max-pool and the plain max-pool, under the
contract of tests/_encoder_eval_ref.py (fp64 ATen chain as the yardstick, the fp32 chain beside it); the pooled map bit
for bit F.max_pool2d of the kernel's own f0, f0 bit for bit mode 1 of the plain kernel; the per-channel vectors unchanged;
two calls (the second with the simulator's threads and workgroups in reverse order) giving the same bits; and guard bands
around every output (tests/_hostsim_enceval.py).  Every shape of the GPU file runs here too: the simulator takes half a
second on the largest."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _encoder_eval_ref as R
import _hostsim_enceval as HS

BN_SHAPES = R.BN_SHAPES
POOL_SHAPES = R.POOL_SHAPES + [(1, 2, 5, 263), (1, 2, 9, 130)]   # (and two odd ones)


def _vectors(case):
    return [case[k].numpy().astype(np.float32) for k in ("gamma", "beta", "running_mean", "running_var")]


def _t(a):
    return torch.from_numpy(np.asarray(a))


def _bn(case):
    vec = _vectors(case)
    before = [v.copy() for v in vec]
    identity = None if case["identity"] is None else case["identity"].numpy()
    y = HS.bn(case["x"].numpy(), identity, *vec, case["mode"], R.EPS)
    for a, b, name in zip(vec, before, ("gamma", "beta", "running_mean", "running_var")):
        assert np.array_equal(a.view(np.int32), b.view(np.int32)), f"{name} was written"
    return _t(y)


def _stem(case):
    vec = _vectors(case)
    before = [v.copy() for v in vec]
    f0, pooled = HS.bn_relu_pool(case["x"].numpy(), *vec, R.EPS)
    for a, b, name in zip(vec, before, ("gamma", "beta", "running_mean", "running_var")):
        assert np.array_equal(a.view(np.int32), b.view(np.int32)), f"{name} was written"
    return _t(f0), _t(pooled)


@pytest.mark.parametrize("special", [False, True], ids=["finite", "nan_inf"])
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("shape", BN_SHAPES)
def test_bn_act_meets_the_contract(shape, mode, special, monkeypatch):
    case = R.make_case(shape, mode, seed=sum(shape) + mode, special=special)
    monkeypatch.delenv("HOSTSIM_ORDER", raising=False)
    y = _bn(case)
    monkeypatch.setenv("HOSTSIM_ORDER", "reverse")
    assert R.same_bits(y, _bn(case)), "two calls differ"
    if special:
        assert int(torch.isnan(y).sum()) == 1 and bool(torch.isnan(y[0, 0, 0, 0]))
    R.check_eval_contract(f"hostsim eval {R.MODES[mode]} {shape}", dict(y=y), R.aten_chain(case, torch.float32),
                          R.aten_chain(case, torch.float64))


def test_eps_carries_the_channel_without_variance():
    case = R.make_case((2, 5, 3, 3), 0, seed=2)
    c = case["zero_var"]
    assert float(case["running_var"][c]) == 0.0
    y = _bn(case)[:, c].double()
    want = (case["x"][:, c] - case["running_mean"][c]) / np.sqrt(np.float32(R.EPS)) * case["gamma"][c] + case["beta"][c]
    assert bool(torch.isfinite(y).all()) and float((y - want).abs().max()) <= 8 * R.U * float(want.abs().max())


@pytest.mark.parametrize("special", [False, True], ids=["finite", "nan_inf"])
@pytest.mark.parametrize("shape", POOL_SHAPES)
def test_stem_meets_the_contract_and_pools_its_own_f0(shape, special, monkeypatch):
    case = R.make_case(shape, 1, seed=sum(shape), special=special)
    monkeypatch.delenv("HOSTSIM_ORDER", raising=False)
    f0, pooled = _stem(case)
    monkeypatch.setenv("HOSTSIM_ORDER", "reverse")
    again = _stem(case)
    assert R.same_bits(f0, again[0]) and R.same_bits(pooled, again[1]), "two calls differ"
    assert R.same_bits(f0, _bn(case)), "f0 is not mode 1 of the plain kernel"
    assert R.same_bits(pooled, F.max_pool2d(f0, 3, 2, 1)), "pooled is not max_pool2d(f0)"
    assert R.same_bits(pooled, _t(HS.maxpool(f0.numpy()))), "the plain pool differs from the fused one"
    R.check_eval_contract(f"hostsim eval stem {shape}", dict(y=f0, pooled=pooled),
                          R.aten_chain(case, torch.float32, pool=True), R.aten_chain(case, torch.float64, pool=True))


@pytest.mark.parametrize("shape", POOL_SHAPES + [(1, 1, 2, 3), (2, 1, 3, 4)])
def test_max_pool_is_bit_identical_to_aten(shape):
    gen = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(shape, generator=gen)
    x = torch.round(x * 2) / 2   # ties in most windows, negative entries (no ReLU in front of this entry point)
    assert R.same_bits(_t(HS.maxpool(x.numpy())), F.max_pool2d(x, 3, 2, 1))


def test_max_pool_nan_wins():
    x = torch.zeros(1, 1, 5, 8)
    x[0, 0, 2, 2] = float("nan")
    x[0, 0, 0, 0] = 3.0
    x[0, 0, 4, 7] = float("inf")
    x[0, 0, 3, 5] = float("-inf")
    assert R.same_bits(_t(HS.maxpool(x.numpy())), F.max_pool2d(x, 3, 2, 1))
    assert R.same_bits(_t(HS.maxpool(x[..., :7].numpy())), F.max_pool2d(x[..., :7].contiguous(), 3, 2, 1))
