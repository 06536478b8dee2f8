"""The judgement shared by the simulator and the GPU tests of scsfm_odom_eval / scsfm_odom_chain against the numpy oracle
(tests/odom_eval_oracle.py).

What must be exact: the number of segments, their first frames, lengths and speeds (so the end frames: the speed is
L / (0.1 (last - first + 1))) and the per-length counts.

What may differ, and by how much.  eps = 2^-53.  Kernel and oracle part only where
 (a) a float64 sum is reduced in another order.  n terms: each order is within (n - 1) eps sum|x| of the exact sum, the
     two within 2 n eps sum|x| of each other.  The short sums count too: the oracle multiplies and inverts poses with
     BLAS / LAPACK (4-term dot products, possibly fused; LU with pivoting), the kernels with the written-out 3-term dot
     products and the adjugate.  An entry of a pose error is at most 16 such roundings deep (three products, three
     inverses), the entries of the rotations are <= 1 and the translations <= max|p|: the two evaluations are within
     BASE = 64 eps of each other on a rotation entry or a cosine and 64 eps max|p| on a translation.
 (b) acos: from another library (glibc's under numpy and the simulator, the device library's on the GPU), each within
     2 ulp: 4 eps acos(d) between them; and, the cosine d having moved by dd, |acos(d -+ dd) - acos(d)| evaluated on the
     data (acos is monotonic).  This is the eps / sqrt(1 - d^2) of a cosine near 1 without its singularity at d = 1.
Propagation of (a) through the alignment:
  scale:    c = sum(XY) / sum(X^2): dc / c <= 2 (3n) eps (sum|XY| / |sum XY| + 1).
  Umeyama:  |dC|_F <= 2 n eps (1 / n) sum |y - my| |x - mx| (+ 64 eps |C|_F for the SVD itself: Jacobi here, LAPACK
            there, both backward stable); the singular values move by at most |dC|_F each; the rotation of the polar /
            Kabsch factor by |dr|_F <= 2 |dC|_F / (d1 + s d2) (the two smallest singular values, the last with the
            reflection's sign; undetermined when that gap vanishes); sigma_x by 2 n eps relative; the means by
            2 n eps mean|x|; so dc / c <= 2 n eps + 3 |dC|_F / (d0 + d1 + s d2),
            |dt| <= |dmy| + c (|dmx| + (dc / c + |dr|) |mx|).
  An aligned position p' = c r p + t then moves by at most  dpos = (dc / c + |dr|) max|p' - t| + |dt|,
  and an entry of the aligned rotation by |dr|  (plus the BASE terms).
Propagation into the errors:
  The segment and RPE errors are built on inv(P_a) P_b, in which r and t cancel: only c reaches their translation,
  |d t_err| <= (dc / c) 2 max|p'| + 64 eps max|p'|; their cosine moves by BASE only.
  ATE is an RMS of |g - p'|: it moves by at most dpos + 64 eps max|p|.
  A mean of m values reduced in another order: 2 m eps relative on top (all terms are non-negative).
The chain: G_k is a product of k inverses; re-associating it (and numpy's product for the written-out one) moves a
position by at most k eps max|position| (2e-10 m on 1,591 frames of 630 m) and a rotation entry by k eps."""
from __future__ import annotations

import numpy as np

import odom_eval_oracle as O

EPS = 2.0 ** -53
BASE = 64 * EPS


def acos_bound(d, dd):
    d = np.asarray(d, np.float64)
    lo, hi = np.clip(d - dd, -1.0, 1.0), np.clip(d + dd, -1.0, 1.0)
    a = np.arccos(d)
    return np.maximum(np.abs(np.arccos(lo) - a), np.abs(np.arccos(hi) - a)) + 4 * EPS * a


def alignment_bounds(ref, alignment):
    """-> (dc_rel, dr, dpos, dd) for one sequence's oracle result."""
    g, p = ref["gt_rel"], ref["aligned"]
    n = len(g)
    if alignment is None or n < 2:
        return 0.0, 0.0, 0.0, BASE
    Y, Xa = g[:, :, 3], p[:, :, 3]
    c = ref["summary"][5]
    if alignment == "scale":
        X = Xa / c
        dc = 2 * 3 * n * EPS * (np.abs(X * Y).sum() / abs((X * Y).sum()) + 1.0)
        return dc, 0.0, dc * np.abs(Xa).max(), BASE
    info = ref["info"]
    d, s3, mx, my = info["d"], info["s3"], info["mean_x"], info["mean_y"]
    r, t = info["r"], info["t"]
    X = (np.linalg.solve(r, (Xa - t).T).T if alignment in ("7dof", "6dof") else Xa) / c  # the re-based prediction
    dC = 2 * n * EPS * np.mean(np.linalg.norm(Y - my, axis=1) * np.linalg.norm(X - mx, axis=1)) \
        + 64 * EPS * np.linalg.norm(info["cov"])
    gap = d[1] + s3 * d[2]
    dr = 2 * dC / gap if gap > 64 * EPS * d[0] else np.inf  # (a straight or two-point trajectory leaves r undetermined)
    dc = 2 * n * EPS + 3 * dC / (d[0] + d[1] + s3 * d[2]) if alignment != "6dof" else 0.0
    dmx, dmy = 2 * n * EPS * np.abs(X).mean(0), 2 * n * EPS * np.abs(Y).mean(0)
    dt = np.linalg.norm(dmy) + c * (np.linalg.norm(dmx) + (dc + dr) * np.linalg.norm(mx))
    if alignment == "scale_7dof":
        return dc, 0.0, dc * np.abs(Xa).max(), BASE
    return dc, dr, (dc + dr) * np.linalg.norm(Xa - t, axis=1).max() + dt, BASE


def check_sequence(out, s, ref, alignment, report=None):
    """out: the library's outputs for a set (dict as tests/_hostsim_odom.evaluate returns); s: the sequence's index;
    ref: the oracle's result for that sequence."""
    n = len(ref["gt_rel"])
    m = len(ref["seg"])
    dc, dr, dpos, dd = alignment_bounds(ref, alignment)
    pmax = float(np.abs(ref["aligned"][:, :, 3]).max())
    gmax = float(np.abs(ref["gt_rel"][:, :, 3]).max())
    dterr = dc * 2 * pmax + BASE * max(pmax, gmax)
    dpos = dpos + BASE * pmax
    dr = dr + BASE
    assert out["n_seg"][s] == m
    seg = out["seg"][s]
    np.testing.assert_array_equal(seg[m:], 0.0)
    seg = seg[:m]
    np.testing.assert_array_equal(seg[:, [0, 3, 4]], ref["seg"][:, [0, 3, 4]])  # first frame, length, speed
    np.testing.assert_array_equal(out["per_length"][s][:, 2], ref["per_length"][:, 2])
    gr = out["gt_rel"][s].reshape(-1, 3, 4)
    assert np.abs(gr[:, :, :3] - ref["gt_rel"][:, :, :3]).max() <= BASE
    assert np.abs(gr[:, :, 3] - ref["gt_rel"][:, :, 3]).max() <= BASE * gmax
    al = out["aligned"][s].reshape(-1, 3, 4)
    finite = np.isfinite(ref["aligned"]).all()
    if finite:
        assert np.abs(al[:, :, :3] - ref["aligned"][:, :, :3]).max() <= dr
        assert np.abs(al[:, :, 3] - ref["aligned"][:, :, 3]).max() <= dpos
    else:  # (a one-frame Umeyama divides by sigma_x = 0: the positions are not finite in either; numpy's 4x4 product
        # also spreads the NaN into the rotation, 0 * NaN, which the kernels' 3x4 product has no term for)
        np.testing.assert_array_equal(np.isfinite(al[:, :, 3]), np.isfinite(ref["aligned"][:, :, 3]))
    L = ref["seg"][:, 3]
    seg_r_tol = acos_bound(ref["seg_cos"], dd) / L if m else np.zeros(0)
    seg_t_tol = dterr / L if m else np.zeros(0)
    assert (np.abs(seg[:, 1] - ref["seg"][:, 1]) <= seg_r_tol).all()
    assert (np.abs(seg[:, 2] - ref["seg"][:, 2]) <= seg_t_tol).all()
    summ, rs = out["summary"][s], ref["summary"]
    assert summ[6] == m
    mean_tol = lambda tol, vals, k: (np.mean(tol) if len(tol) else 0.0) + 2 * k * EPS * (np.mean(vals) if len(vals) else 0)
    tols = [mean_tol(seg_t_tol, ref["seg"][:, 2], m), mean_tol(seg_r_tol, ref["seg"][:, 1], m),
            dpos + BASE * gmax + 2 * n * EPS * rs[2],
            mean_tol(np.full(max(n - 1, 0), dterr), ref["rpe_terms"][0], n),
            mean_tol(acos_bound(ref["rpe_terms"][2], dd), ref["rpe_terms"][1], n),
            dc * abs(rs[5])]
    names = ("t_err", "r_err", "ate", "rpe_t", "rpe_r", "scale")
    for k, name in enumerate(names):
        if np.isnan(rs[k]):
            assert np.isnan(summ[k]), name
            continue
        err = abs(summ[k] - rs[k])
        if report is not None:
            report.append((alignment, s, name, err, tols[k]))
        assert err <= tols[k], (alignment, s, name, err, tols[k])
    for k in range(8):
        sel = L == O.LENGTHS[k]
        for col, c_ref, tol in ((0, 2, seg_t_tol), (1, 1, seg_r_tol)):
            want = ref["per_length"][k, col]
            assert abs(out["per_length"][s][k, col] - want) <= mean_tol(tol[sel], ref["seg"][sel, c_ref], int(sel.sum()))


def check_set(out, gts, preds, alignment, report=None):
    refs = O.evaluate(gts, preds, alignment)
    for s, ref in enumerate(refs):
        check_sequence(out, s, ref, alignment, report)
    return refs


def check_chain(poses, local, report=None):
    """poses [n + 1, 3, 4] from the library against the sequential fold of the library's own local matrices, inverted
    as the kernel inverts them (the bound is the association's, not an inverse's)."""
    f = O.fold(local, O.adjugate_inverse)
    n = len(local)
    np.testing.assert_array_equal(poses[0], np.eye(4)[:3])
    tol_pos = n * EPS * max(float(np.abs(f[:, :, 3]).max()), 0.0)
    err_pos = float(np.abs(poses[:, :, 3] - f[:, :, 3]).max())
    err_rot = float(np.abs(poses[:, :, :3] - f[:, :, :3]).max())
    if report is not None:
        report.append((n, err_pos, tol_pos, err_rot, n * EPS))
    assert err_pos <= tol_pos and err_rot <= n * EPS, (n, err_pos, tol_pos, err_rot)
    return f
