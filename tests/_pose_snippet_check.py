"""The judgement shared by the simulator's and the GPU's snippet tests, and their seeded ragged set.

Tolerances.  Oracle and kernels run the same written-out float64 statements, so they differ only where a library
function does (sqrt, atan2, the division's rounding): rtol 1e-12, the project's number for this class of arithmetic
(tests/test_odom_eval_reference.py).  Two quantities need more than a relative term:
  RE      atan2(s, c) near the identity carries cancellation in s.  max |RE_oracle - RE_reference| measured on the four
          fixtures of tests/golden/pose_snippets.npz on the CPU is 5.64e-17; 8 x that is allowed on top of rtol 1e-12,
          for other BLAS / libm builds: RE_ATOL = 4.6e-16.
  gt      an entry of the compensated ground truth is a dot product of three terms, and a rotation entry of 1e-5 that
          is the difference of products of size 1 has no relative accuracy of its own: the 1e-12 is taken of the entry's
          sum of absolute products (|inv R0| |X|)_ij, the forward-error scale of a dot product, which is the entry's own
          magnitude wherever nothing cancels.
The predictions: rtol 1e-12 with atol 1e-15 (exact zeros and ones in the first pose, tiny rotation entries after)."""
import numpy as np

import odom_eval_oracle as O
import pose_snippet_oracle as P

RTOL = 1e-12
RE_MEASURED = 5.64e-17
RE_ATOL = 4.6e-16  # 8 x RE_MEASURED, rounded up
RAGGED_LENGTHS = (0, 4, 5, 6, 68, 69, 260, 261)  # at seq_len 5: 0, 0, 1, 2, 64, 65, 256, 257 snippets


def check_errors(got, want, report=None):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape
    if report is not None and len(want):
        report.append(("ATE rel", float(np.max(np.abs(got[:, 0] - want[:, 0]) / np.abs(want[:, 0]))),
                       "RE abs", float(np.max(np.abs(got[:, 1] - want[:, 1])))))
    np.testing.assert_allclose(got[:, 0], want[:, 0], rtol=RTOL, atol=0)
    np.testing.assert_allclose(got[:, 1], want[:, 1], rtol=RTOL, atol=RE_ATOL)


def check_pred(got, want):
    np.testing.assert_allclose(got, want, rtol=RTOL, atol=1e-15)


def gt_scale(windows):
    """[N, L, 3, 4] raw ground-truth windows -> the sum of absolute products behind every entry of the compensated
    ground truth."""
    R0inv = np.abs(P.inv3(windows[:, 0, :, :3]))[:, None]
    scale = np.empty(windows.shape)
    scale[..., :3] = P.mul3(R0inv, np.abs(windows[..., :3]))
    scale[..., 3] = P.matvec(R0inv, np.abs(windows[..., 3] - windows[:, :1, :, 3]))
    return scale


def check_gt(got, want, gts, L):
    """got, want [N, L, 3, 4]; gts: the raw sequences they were cut from."""
    wins = [P.windows(np.asarray(g, np.float64).reshape(-1, 3, 4), L) for g in gts if len(g) >= L]
    scale = gt_scale(np.concatenate(wins))
    assert got.shape == want.shape == scale.shape
    assert (np.abs(got - want) <= RTOL * scale).all(), float(np.max(np.abs(got - want) / np.maximum(scale, 1e-300)))


def ragged_set(dtype=np.float64, seed=11):
    """Seeded pair vectors in the style of test_chain_poses (small rotations, 0.4 forward per frame) for RAGGED_LENGTHS
    frames, and as ground truth the oracle's fold of OTHER seeded vectors.  -> (vecs, gts [n, 12])."""
    rng = np.random.default_rng(seed)
    vecs, gts = [], []
    for n in RAGGED_LENGTHS:
        m = max(n - 1, 0)
        v = rng.normal(0.0, 0.01, (m, 6))
        v[:, 2] -= 0.4
        w = rng.normal(0.0, 0.01, (m, 6))
        w[:, 2] -= 1.1
        vecs.append(v.astype(dtype))
        gts.append(O.fold(O.euler_mat(w)).reshape(-1, 12)[:n])
    return vecs, gts
