"""Numpy oracle of KITTI odometry evaluation and of test_vo.py's pose fold, float64 throughout.  Written from the
behaviour include/scsfm_odom.h documents.  Poses are multiplied and inverted as 4x4 matrices with numpy (``@``,
np.linalg.inv: the general inverse), the sums are numpy's (np.sum / np.mean: pairwise), the cumulative distance is the
sequential loop, the rotation error uses Python's min / max, and the 3x3 SVD is LAPACK's.
Test infrastructure; never imported by the product."""
from __future__ import annotations

import math
import warnings

import numpy as np

LENGTHS = (100, 200, 300, 400, 500, 600, 700, 800)
STEP = 10
ALIGNMENTS = (None, "scale", "scale_7dof", "7dof", "6dof")


# ---- affine maps: (A [..., 3, 3], t [..., 3]) ----

def split(P):
    P = np.asarray(P, np.float64)
    if P.shape[-1] == 12:
        P = P.reshape(P.shape[:-1] + (3, 4))
    return P[..., :3].copy(), P[..., 3].copy()


def join(A, t):
    return np.concatenate([A, t[..., None]], axis=-1)


def _mat4(x):
    A, t = x
    M = np.zeros(A.shape[:-2] + (4, 4))
    M[..., :3, :3], M[..., :3, 3], M[..., 3, 3] = A, t, 1.0
    return M


def _aff(M):
    return M[..., :3, :3].copy(), M[..., :3, 3].copy()


def amul(x, y):
    """The 4x4 product, as the reference's ``@``."""
    return _aff(_mat4(x) @ _mat4(y))


def ainv(x):
    """The 4x4 inverse, as the reference's np.linalg.inv."""
    return _aff(np.linalg.inv(_mat4(x)))


def adjugate_inverse(x):
    """The general inverse written out as include/scsfm_odom.h states it: adjugate / determinant, -(A^-1 t)."""
    A, t = x
    a = [A[..., i, j] for i in range(3) for j in range(3)]
    c0, c1, c2 = a[4] * a[8] - a[5] * a[7], a[5] * a[6] - a[3] * a[8], a[3] * a[7] - a[4] * a[6]
    det = (a[0] * c0 + a[1] * c1) + a[2] * c2
    Z = np.empty(A.shape)
    Z[..., 0, 0], Z[..., 1, 0], Z[..., 2, 0] = c0 / det, c1 / det, c2 / det
    Z[..., 0, 1] = (a[2] * a[7] - a[1] * a[8]) / det
    Z[..., 1, 1] = (a[0] * a[8] - a[2] * a[6]) / det
    Z[..., 2, 1] = (a[1] * a[6] - a[0] * a[7]) / det
    Z[..., 0, 2] = (a[1] * a[5] - a[2] * a[4]) / det
    Z[..., 1, 2] = (a[2] * a[3] - a[0] * a[5]) / det
    Z[..., 2, 2] = (a[0] * a[4] - a[1] * a[3]) / det
    z = np.empty(t.shape)
    for i in range(3):
        z[..., i] = -((Z[..., i, 0] * t[..., 0] + Z[..., i, 1] * t[..., 1]) + Z[..., i, 2] * t[..., 2])
    return Z, z


def sel(x, idx):
    return x[0][idx], x[1][idx]


def rot_cos(E):
    A = E[0]
    d = 0.5 * (((A[..., 0, 0] + A[..., 1, 1]) + A[..., 2, 2]) - 1.0)
    d = np.where(1.0 < d, 1.0, d)   # Python's min(d, 1.0): a NaN stays
    return np.where(-1.0 > d, -1.0, d)


def rot_err(E):
    return np.arccos(rot_cos(E))


def trans_err(E):
    t = E[1]
    return np.sqrt((t[..., 0] * t[..., 0] + t[..., 1] * t[..., 1]) + t[..., 2] * t[..., 2])


# ---- test_vo.py ----

def euler_mat(vec):
    """pose_vec2mat(vec, 'euler') in vec's precision with separate roundings: [n, 6] -> [n, 3, 4]."""
    v = np.asarray(vec)
    T = v.dtype.type
    sx, cx, sy, cy, sz, cz = (f(v[:, k]).astype(T) for k in (3, 4, 5) for f in (np.sin, np.cos))
    M = np.empty((len(v), 3, 4), T)
    M[:, 0, 0], M[:, 0, 1], M[:, 0, 2] = cy * cz, -cy * sz, sy
    M[:, 1, 0], M[:, 1, 1], M[:, 1, 2] = cx * sz + sx * sy * cz, cx * cz - sx * sy * sz, -sx * cy
    M[:, 2, 0], M[:, 2, 1], M[:, 2, 2] = sx * sz - cx * sy * cz, sx * cz + cx * sy * sz, cx * cy
    M[:, :, 3] = v[:, :3]
    return M


def quat_mat(vec):
    v = np.asarray(vec)
    T = v.dtype.type
    qx, qy, qz = v[:, 3], v[:, 4], v[:, 5]
    n = np.sqrt(T(1) + qx * qx + qy * qy + qz * qz)
    w, x, y, z = T(1) / n, qx / n, qy / n, qz / n
    M = np.empty((len(v), 3, 4), T)
    M[:, 0, 0], M[:, 0, 1], M[:, 0, 2] = w * w + x * x - y * y - z * z, 2 * x * y - 2 * w * z, 2 * w * y + 2 * x * z
    M[:, 1, 0], M[:, 1, 1], M[:, 1, 2] = 2 * w * z + 2 * x * y, w * w - x * x + y * y - z * z, 2 * y * z - 2 * w * x
    M[:, 2, 0], M[:, 2, 1], M[:, 2, 2] = 2 * x * z - 2 * w * y, 2 * w * x + 2 * y * z, w * w - x * x - y * y + z * z
    M[:, :, 3] = v[:, :3]
    return M


def fold(mats, inverse=ainv):
    """test_vo.py's loop: G_0 = I, G_k = G_{k-1} inv(T_k) in float64, one after the other.  [n, 3, 4] -> [n + 1, 3, 4].
    ``inverse``: np.linalg.inv as the reference (ainv) or the header's written-out one (adjugate_inverse), so that a
    scan of the same inverted matrices differs from this by its association only."""
    A, t = split(np.asarray(mats, np.float64))
    Ai, ti = inverse((A, t))
    g = (np.eye(3), np.zeros(3))
    out = [join(*g)]
    for k in range(len(A)):
        g = amul(g, (Ai[k], ti[k]))
        out.append(join(*g))
    return np.stack(out)


# ---- KittiEvalOdom.eval ----

def rebase(P):
    x = split(P)
    return amul(ainv(sel(x, slice(0, 1))), x)


def distances(g):
    pos = g[1]
    dist = [0.0]
    for i in range(len(pos) - 1):
        dx, dy, dz = pos[i] - pos[i + 1]
        dist.append(dist[i] + math.sqrt((dx * dx + dy * dy) + dz * dz))
    return np.array(dist)


def umeyama(x, y, with_scale):
    """Umeyama's least-squares similarity between the point sets x, y [n, 3] -> r [3, 3], t [3], c, and the pieces the
    tests' bounds need."""
    n = len(x)
    mean_x, mean_y = x.mean(0), y.mean(0)
    dx, dy = x - mean_x, y - mean_y
    sigma_x = 1.0 / n * np.linalg.norm(dx) ** 2
    cov = 1.0 / n * np.sum(dy[:, :, None] * dx[:, None, :], 0)
    u, d, vt = np.linalg.svd(cov)
    s = np.eye(3)
    if np.linalg.det(u) * np.linalg.det(vt) < 0.0:
        s[2, 2] = -1.0
    r = u.dot(s).dot(vt)
    c = np.float64(1.0) / sigma_x * np.trace(np.diag(d).dot(s)) if with_scale else 1.0
    t = mean_y - c * r.dot(mean_x)
    return r, t, c, dict(d=d, s3=s[2, 2], sigma_x=sigma_x, mean_x=mean_x, mean_y=mean_y, cov=cov)


def align(g, p, alignment):
    """-> (aligned prediction, scale, info)"""
    A, t = p[0].copy(), p[1].copy()
    info = {}
    if alignment is None:
        return (A, t), 1.0, info
    if alignment == "scale":
        c = np.sum(t * g[1]) / np.sum(t * t)
        return (A, t * c), float(c), info
    r, tr, c, info = umeyama(t, g[1], alignment != "6dof")
    t = t * c
    if alignment in ("7dof", "6dof"):
        A, t = amul((r, tr), (A, t))
    return (A, t), float(c), dict(info, r=r, t=tr)


def evaluate_sequence(gt, pred, alignment=None):
    """gt, pred: [n, 12] or [n, 3, 4] -> dict(seg [m, 5], last [m], summary [7], per_length [8, 3], aligned, gt_rel,
    dist, info)."""
    assert alignment in ALIGNMENTS
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        g, p = rebase(gt), rebase(pred)
        n = len(g[0])
        dist = distances(g)
        p, scale, info = align(g, p, alignment)
        first, last, length = [], [], []
        for f in range(0, n, STEP):
            for L in LENGTHS:
                hit = np.flatnonzero(dist[f:] > dist[f] + L)
                if len(hit):
                    first.append(f), last.append(f + int(hit[0])), length.append(L)
        first, last = np.array(first, np.int64), np.array(last, np.int64)
        length = np.array(length, np.float64)
        if len(first):
            dg = amul(ainv(sel(g, first)), sel(g, last))
            dp = amul(ainv(sel(p, first)), sel(p, last))
            E = amul(ainv(dp), dg)
            r, t = rot_err(E) / length, trans_err(E) / length
            speed = length / (0.1 * ((last - first) + 1.0))
            seg = np.stack([first.astype(np.float64), r, t, length, speed], 1)
            seg_cos = rot_cos(E)
        else:
            seg, seg_cos = np.zeros((0, 5)), np.zeros(0)
        per_length = np.zeros((len(LENGTHS), 3))
        for k, L in enumerate(LENGTHS):
            m = seg[:, 3] == L
            if m.any():
                per_length[k] = np.mean(seg[m, 2]), np.mean(seg[m, 1]), m.sum()
        ave_t = np.sum(seg[:, 2]) / len(seg) if len(seg) else 0.0
        ave_r = np.sum(seg[:, 1]) / len(seg) if len(seg) else 0.0
        e = g[1] - p[1]
        e = np.sqrt((e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2])
        ate = np.sqrt(np.mean(e * e))
        if n > 1:
            i = np.arange(n - 1)
            E = amul(ainv(amul(ainv(sel(g, i)), sel(g, i + 1))), amul(ainv(sel(p, i)), sel(p, i + 1)))
            rpe_terms = (trans_err(E), rot_err(E), rot_cos(E))
            rpe_t, rpe_r = np.mean(rpe_terms[0]), np.mean(rpe_terms[1])
        else:
            rpe_terms = (np.zeros(0), np.zeros(0), np.zeros(0))
            rpe_t = rpe_r = np.nan
    return dict(seg=seg, last=last, summary=np.array([ave_t, ave_r, ate, rpe_t, rpe_r, scale, float(len(seg))]),
                per_length=per_length, aligned=join(*p), gt_rel=join(*g), dist=dist, info=info, seg_cos=seg_cos,
                ate_terms=e, rpe_terms=rpe_terms)


def evaluate(gts, preds, alignment=None):
    return [evaluate_sequence(g, p, alignment) for g, p in zip(gts, preds)]


# ---- the reference's text ----

def _num(x):
    return str(np.float64(x))


def console_lines(seq, summary):
    t, r, ate, rpe_t, rpe_r, _, m = summary
    return ["Sequence: " + str(seq),
            "Translational error (%):  " + (_num(t * 100) if m else "0"),
            "Rotational error (deg/100m):  " + (_num(r / np.pi * 180 * 100) if m else "0.0"),
            "ATE (m):  " + _num(ate),
            "RPE (m):  " + _num(rpe_t),
            "RPE (deg):  " + _num(rpe_r * 180 / np.pi)]


def copy_block(summaries):
    out = ["-------------------- For Copying ------------------------------"]
    for s in summaries:
        out += ["{0:.2f}".format(s[0] * 100), "{0:.2f}".format(s[1] / np.pi * 180 * 100)]
    return out


def result_txt(seqs, summaries):
    out = ""
    for seq, (t, r, ate, rpe_t, rpe_r, _, _) in zip(seqs, summaries):
        out += "Sequence: \t {} \n".format(seq)
        out += "Trans. err. (%): \t {:.3f} \n".format(t * 100)
        out += "Rot. err. (deg/100m): \t {:.3f} \n".format(r / np.pi * 180 * 100)
        out += "ATE (m): \t {:.3f} \n".format(ate)
        out += "RPE (m): \t {:.3f} \n".format(rpe_t)
        out += "RPE (deg): \t {:.3f} \n\n".format(rpe_r * 180 / np.pi)
    return out


def segment_lines(seg):
    """errors/NN.txt: first frame and length as integers, the speed as Python's float, the errors as numpy's."""
    return "".join("{} {} {} {} {}\n".format(int(f), _num(r), _num(t), int(L), repr(float(v))) for f, r, t, L, v in seg)
