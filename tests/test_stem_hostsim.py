"""The fused stem kernels (csrc_stem/) on the host simulator: the forward bit for bit against the unfused pair of
csrc_enc/ (BatchNorm + ReLU, then the max-pool) on the same simulator, the backward against that pair (dgamma / dbeta
within one ulp, dx within the bound of tests/_stem_ref.py) and against torch-CPU autograd under the contract of
tests/_encoder_ref.py; also with the simulator's threads and workgroups run in reverse order (a result that changes is a
race), and with every output pre-filled with NaN."""
import numpy as np
import pytest
import torch

import _encoder_ref as R
import _hostsim_enc as HE
import _hostsim_stem as HS
import _stem_ref as SR

SHAPES = SR.SMALL_SHAPES


def _np(case, k):
    return case[k].numpy().astype(np.float32)


def _fresh(case):
    return _np(case, "running_mean"), _np(case, "running_var"), np.zeros(1, np.int64)


def _pair_forward(case, x=None):
    x = _np(case, "x") if x is None else x
    rm, rv, nbt = _fresh(case)
    f0, stat = HE.bn_fwd(x, None, _np(case, "gamma"), _np(case, "beta"), rm, rv, nbt, 1, R.EPS, R.MOMENTUM)
    out, arg = HE.maxpool_fwd(f0)
    return dict(f0=f0, out=out, arg=arg, stat=stat, running_mean=rm, running_var=rv, nbt=nbt)


def _stem_forward(case, x=None, n_forward=1):
    x = _np(case, "x") if x is None else x
    rm, rv, nbt = _fresh(case)
    for _ in range(n_forward):
        f0, out, arg, stat = HS.fwd(x, _np(case, "gamma"), _np(case, "beta"), rm, rv, nbt, R.EPS, R.MOMENTUM)
    return dict(f0=f0, out=out, arg=arg, stat=stat, running_mean=rm, running_var=rv, nbt=nbt)


def _same_bits(a, b, what):
    for k in a:
        x, y = a[k], b[k]
        if x.dtype == np.float32:
            x, y = x.view(np.int32), y.view(np.int32)
        assert x.shape == y.shape and np.array_equal(x, y), (what, k)


@pytest.mark.parametrize("order", ["forward", "reverse"])
@pytest.mark.parametrize("shape", SHAPES)
def test_forward_is_the_unfused_pair_bit_for_bit(shape, order, monkeypatch):
    if order == "reverse":
        monkeypatch.setenv("HOSTSIM_ORDER", "reverse")
    case = SR.make_case(shape, seed=sum(shape))
    pair, stem = _pair_forward(case), _stem_forward(case)
    _same_bits(pair, stem, shape)
    _same_bits(stem, _stem_forward(case), shape)
    assert int(stem["nbt"][0]) == 1 and not np.isnan(stem["f0"]).any() and int(stem["arg"].max()) <= 8
    if shape[1] > 2:  # the gamma = beta = 0 channel: all-zero windows, the first entry of the clipped window wins
        arg = stem["arg"][:, -1]
        PH, PW = arg.shape[1:]
        want = 3 * (np.arange(PH) == 0)[:, None] + (np.arange(PW) == 0)[None, :]
        assert np.array_equal(arg, np.broadcast_to(want, arg.shape)) and not stem["out"][:, -1].any()
    x = _np(case, "x")
    x[-1, 1, shape[2] // 2, shape[3] // 2] = np.nan  # one NaN: its channel's statistics, and so its plane, are NaN
    _same_bits(_pair_forward(case, x), _stem_forward(case, x), (shape, "nan"))


def _backwards(case, with_f0):
    fw = _stem_forward(case)
    x, gamma, beta = _np(case, "x"), _np(case, "gamma"), _np(case, "beta")
    g_pool, g_f0 = _np(case, "g_pool"), (_np(case, "g") if with_f0 else None)
    dx, dgamma, dbeta = HS.bwd(g_pool, g_f0, fw["arg"], x, gamma, beta, fw["stat"])
    t = HE.maxpool_bwd(g_pool, fw["arg"], x.shape)
    if with_f0:
        t = t + g_f0
    pdx, _, pdgamma, pdbeta = HE.bn_bwd(t, x, None, gamma, beta, fw["stat"], 1)
    tt = lambda a: torch.from_numpy(a)  # noqa: E731
    mean, invstd = fw["stat"][0].astype(np.float64), fw["stat"][1]
    xhat = (x - (mean + fw["stat"][2])[None, :, None, None]) * invstd[None, :, None, None]
    gprime = np.where((fw["f0"] > 0) | np.isnan(fw["f0"]), t, np.float32(0))
    stem = dict(dx=tt(dx), dgamma=tt(dgamma), dbeta=tt(dbeta))
    pair = dict(dx=tt(pdx), dgamma=tt(pdgamma), dbeta=tt(pdbeta))
    aux = dict(gprime=tt(gprime), xhat=tt(xhat), gamma=tt(gamma), invstd=tt(invstd))
    return stem, pair, aux, fw


@pytest.mark.parametrize("order", ["forward", "reverse"])
@pytest.mark.parametrize("with_f0", [True, False])
@pytest.mark.parametrize("shape", SHAPES)
def test_backward_against_the_unfused_pair(shape, with_f0, order, monkeypatch):
    case = SR.make_case(shape, seed=sum(shape) + 1)
    monkeypatch.delenv("HOSTSIM_ORDER", raising=False)
    stem, pair, aux, fw = _backwards(case, with_f0)
    if order == "reverse":
        monkeypatch.setenv("HOSTSIM_ORDER", "reverse")
        again, _, _, _ = _backwards(case, with_f0)
        for k in stem:
            assert np.array_equal(stem[k].numpy().view(np.int32), again[k].numpy().view(np.int32)), k
    assert all(bool(torch.isfinite(v).all()) for v in stem.values()), "an output that was not stored"
    SR.check_backward_against_pair(f"hostsim stem {shape} f0 gradient {with_f0}", stem, pair, aux)
    if not with_f0:  # an absent gradient of f0 is an all-zero one
        x, gamma, beta = _np(case, "x"), _np(case, "gamma"), _np(case, "beta")
        zero = HS.bwd(_np(case, "g_pool"), np.zeros(shape, np.float32), fw["arg"], x, gamma, beta, fw["stat"])
        for a, b in zip(zero, (stem["dx"], stem["dgamma"], stem["dbeta"])):
            assert np.array_equal(a, b.numpy())


def _fused_for_contract(case, n_forward=1):
    t = lambda a: torch.from_numpy(np.asarray(a))  # noqa: E731
    rm, rv, nbt = _fresh(case)
    x, gamma, beta = _np(case, "x"), _np(case, "gamma"), _np(case, "beta")
    out = {}
    for k in range(n_forward):
        f0, pooled, arg, stat = HS.fwd(x, gamma, beta, rm, rv, nbt, R.EPS, R.MOMENTUM)
        if k == 0:
            out["running_mean_1"], out["running_var_1"] = t(rm.copy()), t(rv.copy())
    dx, dgamma, dbeta = HS.bwd(_np(case, "g_pool"), _np(case, "g"), arg, x, gamma, beta, stat)
    out.update(f0=t(f0), pooled=t(pooled), dx=t(dx), dgamma=t(dgamma), dbeta=t(dbeta), mean=t(stat[0]),
               invstd=t(stat[1]), running_mean=t(rm), running_var=t(rv), num_batches_tracked=int(nbt[0]))
    return out


@pytest.mark.parametrize("shape", SHAPES)
def test_backward_against_aten(shape):
    case = SR.make_conditioned_case(shape, seed=sum(shape) + 2)
    assert SR.off_the_kinks(case)
    R.check_contract(f"hostsim stem {shape}", _fused_for_contract(case), SR.aten_chain(case, torch.float32),
                     SR.aten_chain(case, torch.float64))


def test_three_forwards_before_one_backward():
    case = SR.make_conditioned_case((2, 4, 8, 16), seed=11)
    R.check_contract("hostsim stem x3", _fused_for_contract(case, 3), SR.aten_chain(case, torch.float32, 3),
                     SR.aten_chain(case, torch.float64, 3))


def test_argmax_names_atens_winner():
    case = SR.make_case((2, 3, 7, 10), seed=4)
    fw = _stem_forward(case)
    ref, idx = torch.nn.functional.max_pool2d(torch.from_numpy(fw["f0"]), 3, 2, 1, return_indices=True)
    PH, PW = ref.shape[2:]
    ph, pw = np.meshgrid(np.arange(PH), np.arange(PW), indexing="ij")
    arg = fw["arg"].astype(np.int64)
    assert np.array_equal((2 * ph - 1 + arg // 3) * 10 + 2 * pw - 1 + arg % 3, idx.numpy())
    assert np.array_equal(fw["out"].view(np.int32), ref.numpy().view(np.int32))
