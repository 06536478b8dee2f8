"""Numpy oracle of test_pose.py's 5-frame snippet evaluation, float64 throughout, written from the behaviour
include/scsfm_snip.h documents: products and inverses written out entry by entry with the header's association (no
``@``, no np.linalg.inv), the sums over a snippet's translation entries taken frame after frame, left to right.  Every
function works on a stack of snippets at once (leading axis); ``evaluate_sequence_loop`` is the reference's shape of the
work, one snippet after the other.  Test infrastructure; never imported by the product."""
from __future__ import annotations

import numpy as np

import odom_eval_oracle as O


def mats(vec, mode="euler"):
    """pose_vec2mat in vec's precision, lifted to double: [n, 6] -> [n, 3, 4]."""
    return (O.quat_mat(vec) if mode == "quat" else O.euler_mat(vec)).astype(np.float64)


def inv3(A):
    """The general inverse of [..., 3, 3]: adjugate / determinant."""
    a = [A[..., i, j] for i in range(3) for j in range(3)]
    c0, c1, c2 = a[4] * a[8] - a[5] * a[7], a[5] * a[6] - a[3] * a[8], a[3] * a[7] - a[4] * a[6]
    det = (a[0] * c0 + a[1] * c1) + a[2] * c2
    Z = np.empty(np.shape(A))
    Z[..., 0, 0], Z[..., 1, 0], Z[..., 2, 0] = c0 / det, c1 / det, c2 / det
    Z[..., 0, 1] = (a[2] * a[7] - a[1] * a[8]) / det
    Z[..., 1, 1] = (a[0] * a[8] - a[2] * a[6]) / det
    Z[..., 2, 1] = (a[1] * a[6] - a[0] * a[7]) / det
    Z[..., 0, 2] = (a[1] * a[5] - a[2] * a[4]) / det
    Z[..., 1, 2] = (a[2] * a[3] - a[0] * a[5]) / det
    Z[..., 2, 2] = (a[0] * a[4] - a[1] * a[3]) / det
    return Z


def mul3(A, B):
    """[..., 3, 3] x [..., 3, k], every entry (a_i0 b_0j + a_i1 b_1j) + a_i2 b_2j."""
    return (A[..., :, 0, None] * B[..., None, 0, :] + A[..., :, 1, None] * B[..., None, 1, :]) \
        + A[..., :, 2, None] * B[..., None, 2, :]


def matvec(A, v):
    return mul3(A, v[..., None])[..., 0]


def invert(M):
    """inv(A, t) = (A^-1, -(A^-1 t)) for [..., 3, 4]."""
    Ai = inv3(M[..., :3])
    return np.concatenate([Ai, -matvec(Ai, M[..., 3])[..., None]], -1)


def fold(Tinv):
    """[N, L - 1, 3, 4] inverted pair matrices -> [N, L, 3, 4]: P_0 = I, P_i = P_{i-1} Tinv_{i-1}, one after the other."""
    N, m = Tinv.shape[:2]
    P = np.zeros((N, m + 1, 3, 4))
    P[:, 0, :, :3] = np.eye(3)
    for i in range(1, m + 1):
        A, t = P[:, i - 1, :, :3], P[:, i - 1, :, 3]
        Y = Tinv[:, i - 1]
        P[:, i, :, :3] = mul3(A, Y[..., :3])
        P[:, i, :, 3] = matvec(A, Y[..., 3]) + t
    return P


def compensate(gt):
    """test_framework_KITTI.generator's compensation of [N, L, 3, 4]: the first frame's translation subtracted from
    every frame's, then every 3x4 multiplied from the left by the inverse of the first frame's 3x3."""
    R0inv = inv3(gt[:, 0, :, :3])[:, None]
    out = np.empty(gt.shape)
    out[..., :3] = mul3(R0inv, gt[..., :3])
    out[..., 3] = matvec(R0inv, gt[..., 3] - gt[:, :1, :, 3])
    return out


def pose_errors(gt, pred):
    """compute_pose_error for stacks [N, L, 3, 4] -> [N, 2] (ATE, RE); a zero denominator gives numpy's NaN / inf."""
    N, L = gt.shape[:2]
    g, p = gt[..., 3].reshape(N, -1), pred[..., 3].reshape(N, -1)
    with np.errstate(all="ignore"):
        sgp, spp = np.zeros(N), np.zeros(N)
        for k in range(3 * L):
            sgp = sgp + g[:, k] * p[:, k]
            spp = spp + p[:, k] * p[:, k]
        scale = sgp / spp
        sq = np.zeros(N)
        for k in range(3 * L):
            e = g[:, k] - scale * p[:, k]
            sq = sq + e * e
        re = np.zeros(N)
        for i in range(L):
            R = mul3(gt[:, i, :, :3], inv3(pred[:, i, :, :3]))
            d0, d1, d2 = R[:, 0, 1] - R[:, 1, 0], R[:, 1, 2] - R[:, 2, 1], R[:, 0, 2] - R[:, 2, 0]
            s = np.sqrt((d0 * d0 + d1 * d1) + d2 * d2)
            c = ((R[:, 0, 0] + R[:, 1, 1]) + R[:, 2, 2]) - 1.0
            re = re + np.arctan2(s, c)
        return np.stack([np.sqrt(sq) / L, re / L], 1)


def windows(x, L):
    """[n, ...] -> [n - L + 1, L, ...]: window j holds rows j .. j + L - 1 (a copy)."""
    n = len(x)
    idx = np.arange(max(n - L + 1, 0))[:, None] + np.arange(L)[None]
    return np.asarray(x)[idx]


def evaluate_sequence(pair_mats, gt, L=5):
    """pair_mats [n - 1, 3, 4] (pose_vec2mat of the pairs, lifted to double), gt [n, 12] or [n, 3, 4] ->
    dict(pred [N, L, 3, 4], gt [N, L, 3, 4], errors [N, 2]) for the N = max(0, n - L + 1) snippets."""
    gt = np.asarray(gt, np.float64).reshape(-1, 3, 4)
    pair_mats = np.asarray(pair_mats, np.float64).reshape(-1, 3, 4)
    assert len(pair_mats) == max(len(gt) - 1, 0)
    if len(gt) < L:
        return dict(pred=np.zeros((0, L, 3, 4)), gt=np.zeros((0, L, 3, 4)), errors=np.zeros((0, 2)))
    pred = fold(windows(invert(pair_mats), L - 1))
    comp = compensate(windows(gt, L))
    return dict(pred=pred, gt=comp, errors=pose_errors(comp, pred))


def evaluate_sequence_loop(pair_mats, gt, L=5):
    """The same numbers snippet by snippet, as the reference's loop forms them: every snippet inverts its own L - 1
    pairs and folds them."""
    gt = np.asarray(gt, np.float64).reshape(-1, 3, 4)
    pair_mats = np.asarray(pair_mats, np.float64).reshape(-1, 3, 4)
    preds, comps, errs = [], [], []
    for j in range(max(len(gt) - L + 1, 0)):
        pred = fold(invert(pair_mats[j:j + L - 1])[None])
        comp = compensate(gt[None, j:j + L])
        preds.append(pred[0]), comps.append(comp[0]), errs.append(pose_errors(comp, pred)[0])
    return dict(pred=np.array(preds).reshape(-1, L, 3, 4), gt=np.array(comps).reshape(-1, L, 3, 4),
                errors=np.array(errs).reshape(-1, 2))


def evaluate(pair_mats_list, gts, L=5):
    """Several sequences -> the concatenation, in order."""
    outs = [evaluate_sequence(m, g, L) for m, g in zip(pair_mats_list, gts)]
    return {k: np.concatenate([o[k] for o in outs]) for k in ("pred", "gt", "errors")}


def stats(errors):
    """mean ATE, mean RE, std ATE, std RE over the errors rounded to float32 (what the reference's array holds),
    accumulated in double; the population std."""
    e = np.asarray(errors).astype(np.float32).astype(np.float64)
    return np.concatenate([e.mean(0), e.std(0)])


def report_lines(mean, std):
    return ["", "Results", "\t {:>10}, {:>10}".format("ATE", "RE"), "mean \t {:10.4f}, {:10.4f}".format(*mean),
            "std \t {:10.4f}, {:10.4f}".format(*std)]
