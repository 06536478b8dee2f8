"""The one-launch Adam's kernel on the host simulator against the numpy restatement of include/scsfm_opt.h, bit for bit
over five steps: every size around a 16-byte unit, a wave, a workgroup and a chunk, aligned and as views one element on,
a tensor whose gradient is absent in two steps, with and without weight decay, two learning rates, gradients that are 0,
that underflow the second moment, that leave it subnormal and that are huge; sentinels around every segment."""
import numpy as np
import pytest

import _adam_cases as C
import _hostsim_opt as H


@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_five_steps_equal_the_numpy_restatement_bit_for_bit(wd):
    tensors = C.default_tensors()
    assert {t.n for t in tensors} >= set(C.SIZES) and {t.shifted for t in tensors} == {False, True}
    steps = C.run_case(H.lib(), C.HostBackend(), tensors, wd)
    lag = [t for t in tensors if t.lagging]
    assert len(lag) == 1 and lag[0].step == C.STEPS - len(C.ABSENT_IN)
    assert sorted(set(steps)) == [C.STEPS - len(C.ABSENT_IN), C.STEPS]


def test_the_restatement_is_torchs_formula():
    """the yardstick's yardstick: the numpy step against an fp64 Adam written from the paper, to fp32 rounding"""
    rng = np.random.default_rng(1)
    p, g = rng.standard_normal(1000).astype(C.f32), rng.standard_normal(1000).astype(C.f32)
    m, v = np.zeros(1000, C.f32), np.zeros(1000, C.f32)
    p64, m64, v64 = p.astype(np.float64), m.astype(np.float64), v.astype(np.float64)
    for step in (1, 2, 3):
        p, m, v = C.numpy_step(p, g, m, v, *C.host_scalars(1e-3, step), C.f32(0.01))
        g64 = g.astype(np.float64) + 0.01 * p64
        m64 = 0.9 * m64 + 0.1 * g64
        v64 = 0.999 * v64 + 0.001 * g64 * g64
        p64 = p64 - 1e-3 / (1 - 0.9 ** step) * m64 / (np.sqrt(v64) / np.sqrt(1 - 0.999 ** step) + 1e-8)
    assert np.abs(p - p64).max() <= 4 * 2.0 ** -24 * np.abs(p64).max()


def test_the_smoke_shapes():
    C.run_case(H.lib(), C.HostBackend(), C.smoke_tensors(), 0.0, steps=3, absent_in=())
