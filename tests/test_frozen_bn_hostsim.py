"""The frozen-statistics BatchNorm backward (csrc_fbn/) on the host simulator against torch-CPU: dx, d_identity, dgamma and
dbeta of bn [+ residual] [+ ReLU] under the contract of tests/_frozen_bn_ref.py (the fp64 ATen chain as the yardstick, the
fp32 chain beside it), with y taken from the forward the product runs (csrc_enceval/ on the simulator); the no-parameter
form giving the same dx bits and leaving the workspace alone; planted NaN / inf against ATen's bit patterns; two calls
(the second with the simulator's threads and workgroups in reverse order) giving the same bits; an upstream gradient
4 bytes off its alignment taking the scalar path to the same values; the per-channel vectors unchanged; guard bands around
every output and the workspace, which starts out as NaNs (tests/_hostsim_fbn.py)."""
import numpy as np
import pytest
import torch

import _frozen_bn_ref as R
import _hostsim_enceval as HSE
import _hostsim_fbn as HS

NAMES = ("gamma", "beta", "running_mean", "running_var")


def _t(a):
    return torch.from_numpy(np.asarray(a))


def _run(case, **kw):
    """forward by the eval-mode kernel, backward by the frozen one -> dict of tensors (y included)"""
    vec = {k: case[k].numpy().astype(np.float32) for k in NAMES}
    before = {k: v.copy() for k, v in vec.items()}
    x = case["x"].numpy().astype(np.float32)
    identity = None if case["identity"] is None else case["identity"].numpy().astype(np.float32)
    y = HSE.bn(x, identity, *(vec[k] for k in NAMES), case["mode"], R.EPS)
    out = HS.bn_bwd(case["g"].numpy().astype(np.float32), x, y, vec["gamma"], vec["running_mean"], vec["running_var"],
                    case["mode"], R.EPS, **kw)
    for k in NAMES:
        assert np.array_equal(vec[k].view(np.int32), before[k].view(np.int32)), f"{k} was written"
    return {k: _t(v) for k, v in out.items()}


def _same(a, b):
    return a.keys() == b.keys() and all(R.EV.same_bits(a[k], b[k]) for k in a)


@pytest.mark.parametrize("special", [False, True], ids=["finite", "nan_inf"])
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("shape", R.SHAPES)
def test_backward_meets_the_contract(shape, mode, special, monkeypatch):
    case = R.make_case(shape, mode, seed=sum(shape) + mode, special=special)
    monkeypatch.delenv("HOSTSIM_ORDER", raising=False)
    got = _run(case)
    monkeypatch.setenv("HOSTSIM_ORDER", "reverse")
    assert _same(got, _run(case)), "two calls differ"
    assert set(got) == {"dx", "dgamma", "dbeta"} | ({"d_identity"} if mode == 2 else set())
    ref32 = R.aten_chain(case, torch.float32)
    if special and mode:
        # where y is a NaN the gradient passes, here and in ATen (the value is held to the contract below)
        assert float(got["dx"][0, 0, 0, 0]) != 0 and float(ref32["dx"][0, 0, 0, 0]) != 0
    R.check_frozen_contract(f"hostsim frozen {R.MODES[mode]} {shape}", got, ref32, R.aten_chain(case, torch.float64))


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("shape", R.SHAPES)
def test_without_parameter_gradients_same_dx_and_no_workspace(shape, mode):
    case = R.make_case(shape, mode, seed=sum(shape) + mode)
    full = _run(case)
    for spare_ws in (False, True):
        bare = _run(case, params=False, spare_ws=spare_ws)
        assert set(bare) == set(full) - {"dgamma", "dbeta"}
        assert all(R.EV.same_bits(bare[k], full[k]) for k in bare)


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("shape", R.VECTOR_SHAPES)
def test_a_gradient_off_its_alignment_takes_the_scalar_path(shape, mode):
    """the same element-wise bits; the sums are added in the scalar path's order, so they are held to the contract"""
    case = R.make_case(shape, mode, seed=sum(shape) + mode)
    assert R.tasks(shape)[2] and not R.tasks(shape, aligned=False)[2]
    got, off = _run(case), _run(case, misalign=True)
    for k in ("dx", "d_identity"):
        assert k not in got or R.EV.same_bits(got[k], off[k]), k
    R.check_frozen_contract(f"hostsim frozen {R.MODES[mode]} {shape} off by 4 bytes", off,
                            R.aten_chain(case, torch.float32), R.aten_chain(case, torch.float64))


def test_the_cases_are_what_they_claim():
    """the shapes hit the paths they are listed for, and no pre-activation of a case lies on the kink"""
    wave, threads, unroll, max_blocks = R.kernel_constants()
    unit = unroll * wave
    # ((1, 3, 2, 2) is the smallest plane there is on the 16-byte path: one unit; the other three are scalar)
    assert R.tasks(R.SCALAR_SHAPES[0])[2] and all(not R.tasks(s)[2] for s in R.SCALAR_SHAPES[1:])
    assert all(R.tasks(s)[2] for s in R.VECTOR_SHAPES)
    assert 5 * 263 > 2 * unit and (5 * 263) % unit            # several tasks to a plane and a tail
    assert 33 * 32 // 4 > unit and (33 * 32 // 4) % unit == 8  # full tasks and one of 8 units, 32 floats
    B, C, H, W = R.TINY_PLANES
    assert H * W // 4 <= unit and B > 1 and C % (threads // wave) == 0
    for shape in R.SHAPES:
        for mode in (1, 2):
            v = R._preactivation(R.make_case(shape, mode, seed=sum(shape) + mode))
            assert not bool(((v.abs() < R.KINK) & (v != 0)).any())


def test_workspace_bytes():
    wave, threads, unroll, max_blocks = R.kernel_constants()
    for shape in R.SHAPES + [R.STEM_PLANE]:
        B, C, H, W = shape
        assert HS.workspace_bytes(shape) == 16 * R.tasks(shape, aligned=False)[0]
        assert R.tasks(shape, aligned=False)[0] >= R.tasks(shape)[0]
    assert HS.workspace_bytes((0, 1, 1, 1)) == 0 and HS.workspace_bytes((1 << 15, 1 << 8, 1 << 4, 1 << 4)) == 0
