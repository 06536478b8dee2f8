"""The encoder kernels (csrc_enc/) on the host simulator against torch-CPU autograd: fused BatchNorm [+ residual]
[+ ReLU] forward and backward under the contract of tests/_encoder_ref.py (fp64 ATen chain as the yardstick, the fp32
chain beside it), the max-pool bit for bit against ATen; both also with the simulator's threads and workgroups run in
reverse order (a result that changes is a race), and with every output pre-filled with NaN (tests/_hostsim_enc.py)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _encoder_ref as R
import _hostsim_enc as HS

# the odd shapes, and the stage shapes of configs[1] reduced (batch 2, fewer channels, the stages' aspect ratio)
REDUCED = [(2, 8, 16, 52), (2, 6, 8, 26), (2, 16, 4, 12), (3, 70, 2, 6)]


def _run(case, n_forward=1):
    t = lambda a: torch.from_numpy(np.asarray(a))
    mode = case["mode"]
    rm, rv = case["running_mean"].numpy().astype(np.float32), case["running_var"].numpy().astype(np.float32)
    nbt = np.zeros(1, np.int64)
    fused = {}
    for k in range(n_forward):
        y, stat = HS.bn_fwd(case["x"].numpy(), None if case["identity"] is None else case["identity"].numpy(),
                            case["gamma"].numpy(), case["beta"].numpy(), rm, rv, nbt, mode, R.EPS, R.MOMENTUM)
        if k == 0:
            fused["running_mean_1"], fused["running_var_1"] = t(rm.copy()), t(rv.copy())
    dx, d_id, dgamma, dbeta = HS.bn_bwd(case["g"].numpy(), case["x"].numpy(), y, case["gamma"].numpy(),
                                        case["beta"].numpy(), stat, mode)
    fused.update(y=t(y), dx=t(dx), dgamma=t(dgamma), dbeta=t(dbeta), mean=t(stat[0]), invstd=t(stat[1]),
                 running_mean=t(rm), running_var=t(rv), num_batches_tracked=int(nbt[0]))
    if mode == 2:
        fused["d_identity"] = t(d_id)
    return fused


@pytest.mark.parametrize("order", ["forward", "reverse"])
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("shape", R.ODD_SHAPES + REDUCED + R.HOSTSIM_SPLIT_EDGE_SHAPES)
def test_bn_act_meets_the_contract(shape, mode, order, monkeypatch):
    """The last three shapes are edges of the split of a channel over S workgroups (tests/_encoder_ref.py): the cap
    S = 64, and the uneven S = 5 (16-byte path, batch boundaries inside a range) and S = 3 (scalar path).  The S = 43
    shape (2, 48, 128, 172) takes the simulator 4 to 8 s a case and runs on the GPU only
    (tests/test_gpu_encoder_fused.py)."""
    if shape in R.SPLIT_EDGE_SHAPES:
        assert R.splits(shape)[0] == R.SPLIT_EDGE_SHAPES[shape]
    case = R.make_case(shape, mode, seed=sum(shape) + mode)
    monkeypatch.delenv("HOSTSIM_ORDER", raising=False)
    first = _run(case)
    if order == "reverse":
        monkeypatch.setenv("HOSTSIM_ORDER", "reverse")
        fused = _run(case)
        for k, v in first.items():  # the same bits in either order
            assert v == fused[k] if isinstance(v, int) else np.array_equal(v.numpy().view(np.int32),
                                                                           fused[k].numpy().view(np.int32)), k
    else:
        fused = first
    R.check_contract(f"hostsim {R.MODES[mode]} {shape}", fused, R.aten_chain(case, torch.float32),
                     R.aten_chain(case, torch.float64))


def test_split_cases_hit_the_intended_values():
    """the S of every listed shape, recomputed from the constants of csrc_enc/scsfm_encoder.hip: all of 1, 2, 3, 4, 5, 8,
    43 and 64, the uneven ones on both paths"""
    listed = {**R.R50_STAGE_SHAPES, **R.SPLIT_EDGE_SHAPES}
    got = {shape: R.splits(shape) for shape in listed}
    assert {shape: S for shape, (S, _) in got.items()} == listed
    assert sorted(set(listed.values())) == [1, 2, 3, 4, 5, 8, 43, 64]
    assert [shape for shape, (_, vec) in got.items() if not vec] == [(1, 2, 5, 127)]
    assert set(R.HOSTSIM_SPLIT_EDGE_SHAPES) == set(R.SPLIT_EDGE_SHAPES) - {(2, 48, 128, 172)}
    for (B, C, H, W), (S, vec) in got.items():  # uneven: the ranges of units are not all of one length
        units = B * H * W // (4 if vec else 1)
        assert (units % S != 0) == (S in (3, 5)), (B, C, H, W)
    # (3, 4, 4, 401): the batch boundaries at units 401 and 802 lie inside ranges, not between them
    cuts = [1203 * s // 5 for s in range(6)]
    assert 401 not in cuts and 802 not in cuts


@pytest.mark.parametrize("mode", [1, 2])
def test_three_forwards_before_one_backward(mode):
    case = R.make_case((2, 5, 6, 10), mode, seed=11)
    R.check_contract(f"hostsim {R.MODES[mode]} x3", _run(case, 3), R.aten_chain(case, torch.float32, 3),
                     R.aten_chain(case, torch.float64, 3))


def test_relu_mask_is_the_forwards():
    """g' is dropped exactly where the forward's output is not positive: in mode 1 (mask recomputed from x) as in mode
    2 (mask read from y), d_identity / dbeta show it entry for entry"""
    case = R.make_case((2, 4, 5, 7), 2, seed=3)
    out = _run(case)
    want = torch.where(out["y"] > 0, case["g"].float(), torch.zeros(()))
    assert torch.equal(out["d_identity"], want)
    case1 = R.make_case((2, 4, 5, 7), 1, seed=3)
    out1 = _run(case1)
    want1 = torch.where(out1["y"] > 0, case1["g"].float(), torch.zeros(())).double().sum((0, 2, 3))
    assert float((out1["dbeta"].double() - want1).abs().max()) <= 4 * R.U * float(case1["g"].abs().sum())
    assert bool((out1["y"][:, 3] == 0).all()) and float(out1["dbeta"][3]) == 0.0  # the gamma = beta = 0 channel


def test_nan_passes_through_the_relu():
    case = R.make_case((1, 2, 3, 4), 2, seed=5)
    case["identity"][0, 1, 2, 3] = float("nan")
    y = _run(case)["y"]
    assert bool(torch.isnan(y[0, 1, 2, 3])) and int(torch.isnan(y).sum()) == 1


@pytest.mark.parametrize("order", ["forward", "reverse"])
@pytest.mark.parametrize("shape", [(1, 1, 1, 1), (1, 3, 2, 2), (2, 5, 3, 3), (3, 2, 5, 263), (1, 4, 7, 131),
                                   (2, 3, 16, 52), (1, 2, 9, 8)])
def test_max_pool_is_bit_identical_to_aten(shape, order, monkeypatch):
    if order == "reverse":
        monkeypatch.setenv("HOSTSIM_ORDER", "reverse")
    x = R.pool_input(shape, seed=sum(shape)).requires_grad_()
    ref, idx = F.max_pool2d(x, 3, 2, 1, return_indices=True)
    out, arg = HS.maxpool_fwd(x.detach().numpy())
    assert np.array_equal(out.view(np.int32), ref.detach().numpy().view(np.int32))
    # the byte names ATen's winner
    PH, PW = ref.shape[2:]
    ph, pw = np.meshgrid(np.arange(PH), np.arange(PW), indexing="ij")
    h, w = 2 * ph - 1 + arg // 3, 2 * pw - 1 + arg % 3
    assert np.array_equal(h * shape[3] + w, idx.numpy())
    g = torch.randn(ref.shape, generator=torch.Generator().manual_seed(1))
    ref.backward(g)
    dx = HS.maxpool_bwd(g.numpy(), arg, shape)
    assert np.array_equal(dx.view(np.int32), x.grad.numpy().view(np.int32))


def test_max_pool_nan_wins():
    x = torch.zeros(1, 1, 5, 5)
    x[0, 0, 2, 2] = float("nan")
    x[0, 0, 0, 0] = 3.0
    ref, idx = F.max_pool2d(x, 3, 2, 1, return_indices=True)
    out, arg = HS.maxpool_fwd(x.numpy())
    assert np.array_equal(np.isnan(out), torch.isnan(ref).numpy()) and np.array_equal(out[~np.isnan(out)],
                                                                                      ref[~torch.isnan(ref)].numpy())
    ph, pw = np.meshgrid(np.arange(3), np.arange(3), indexing="ij")
    assert np.array_equal((2 * ph - 1 + arg // 3) * 5 + 2 * pw - 1 + arg % 3, idx.numpy())


@pytest.mark.parametrize("order", ["forward", "reverse"])
def test_mode1_mask_is_the_forwards_on_the_kink(order, monkeypatch):
    """The mode-1 backward recomputes the ReLU mask from x.  Here 24 pre-activations per channel lie within a few ulp of
    0 on both sides (x in steps of one ulp around an entry whose bn value beta cancels), one channel has gamma = 0 with
    beta > 0 (everything passes) and one gamma = 0 with beta < 0 (nothing does).  The mask must be the forward's entry
    for entry: with g = 2^k on the k-th kink entry dbeta's bits name exactly the entries that passed, and dx, dgamma,
    dbeta are bitwise those of the plain BatchNorm backward (mode 0) fed g * [y > 0]."""
    if order == "reverse":
        monkeypatch.setenv("HOSTSIM_ORDER", "reverse")
    rng = np.random.default_rng(4)
    B, C, H, W = 2, 4, 6, 16
    x = rng.standard_normal((B, C, H, W)).astype(np.float32)
    kink = np.zeros(x.shape, bool)
    kink[0, :2, 1, :] = True
    kink[1, :2, 2, :8] = True
    for c in range(2):
        v = x[0, c, 0, 0]
        chain = [v]
        for _ in range(12):
            chain.insert(0, np.nextafter(chain[0], np.float32(-np.inf)))
        for _ in range(11):
            chain.append(np.nextafter(chain[-1], np.float32(np.inf)))
        x[:, c][kink[:, c]] = np.array(chain, np.float32)
    fresh = lambda: (np.zeros(C, np.float32), np.ones(C, np.float32), np.zeros(1, np.int64))  # noqa: E731
    one, zero = np.ones(C, np.float32), np.zeros(C, np.float32)
    xh, _ = HS.bn_fwd(x, None, one, zero, *fresh(), 0, R.EPS, R.MOMENTUM)  # fmaf(xhat, 1, 0) = xhat
    gamma = np.array([1.3, -0.7, 0.0, 0.0], np.float32)
    beta = np.array([0, 0, 0.3, -0.3], np.float32)
    for c in range(2):
        beta[c] = -(gamma[c] * xh[:, c][kink[:, c]][12])
    y, stat = HS.bn_fwd(x, None, gamma, beta, *fresh(), 1, R.EPS, R.MOMENTUM)
    for c in range(2):
        on = y[:, c][kink[:, c]]
        assert 0 < int((on > 0).sum()) < 24, "the kink is not straddled"
        assert float(np.abs(on).max()) < 1e-5
    assert np.all(y[:, 2] == np.float32(0.3)) and np.all(y[:, 3] == 0)
    g = np.zeros(x.shape, np.float32)
    for c in range(4):
        g[:, c][kink[:, c % 2]] = 2.0 ** np.arange(24)
    dx, _, dgamma, dbeta = HS.bn_bwd(g, x, None, gamma, beta, stat, 1)
    for c in range(4):
        assert float(dbeta[c]) == float(g[:, c][y[:, c] > 0].astype(np.float64).sum()), c
    assert float(dbeta[2]) == 2.0 ** 24 - 1 and float(dbeta[3]) == 0.0
    for grad in (g, rng.standard_normal(x.shape).astype(np.float32)):
        got = HS.bn_bwd(grad, x, None, gamma, beta, stat, 1)
        want = HS.bn_bwd(np.where(y > 0, grad, np.float32(0)), x, None, gamma, beta, stat, 0)
        for a, b, name in zip(got, want, ("dx", "d_identity", "dgamma", "dbeta")):
            if a is not None:
                assert np.array_equal(a.view(np.int32), b.view(np.int32)), name
