"""include/scsfm_track.h restated in numpy: the yardstick of tests/test_tracking_hostsim.py and tests/test_gpu_tracking.py,
which compare the kernels with it bit for bit.  The pair of a pixel is one numpy operation on np.float32 arrays per
operation of the header (numpy neither fuses a multiply with an add nor flushes denormals, and its division and square
root are correctly rounded); the sums are np.float64 arrays added in the header's tree: a thread's four pixels, the six
butterfly steps of a wave, the four waves, the workgroups in index order; the solve is scalar np.float64.  It takes the
inputs of scsfm_hip.tracking.align.  Test infrastructure only."""
from __future__ import annotations

import numpy as np

f32 = np.float32
f64 = np.float64
TILE, THREADS, WAVE, SUMS = 1024, 256, 64, 29
PIVOT_EPS = 1e-8
PAIRS = [(i, j) for i in range(6) for j in range(i, 6)]


def normalise(q):
    ln = np.sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3])
    return [c / ln for c in q]


def matrix(q):
    """the header's matrix of a quaternion (w, x, y, z), nine np.float64 row-major"""
    w, x, y, z = q
    xx, yy, zz, xy, xz, yz, wx, wy, wz = x * x, y * y, z * z, x * y, x * z, y * z, w * x, w * y, w * z
    one, two = f64(1), f64(2)
    return [one - two * (yy + zz), two * (xy - wz), two * (xz + wy),
            two * (xy + wz), one - two * (xx + zz), two * (yz - wx),
            two * (xz - wy), two * (yz + wx), one - two * (xx + yy)]


def record(state, K=None, old=None):
    """the fp32 pose record of one state [7]; fx fy cx cy from K, or kept from ``old``"""
    rec = np.empty(16, np.float32) if old is None else old.copy()
    rec[:9] = np.array(matrix(state[:4]), np.float64).astype(np.float32)
    rec[9:12] = state[4:7].astype(np.float32)
    if K is not None:
        K = np.asarray(K, np.float32).reshape(9)
        rec[12], rec[13], rec[14], rec[15] = K[0], K[4], K[2], K[5]
    return rec


def init(c2w, K):
    """c2w [V, 12] or [V, 3, 4] float64 -> (state [V, 7] float64, est [V, 16] float32)"""
    c2w = np.asarray(c2w, np.float64).reshape(-1, 3, 4)
    state = np.empty((len(c2w), 7), np.float64)
    est = np.empty((len(c2w), 16), np.float32)
    one, half, two = f64(1), f64(0.5), f64(2)
    with np.errstate(all="ignore"):
        for v, m in enumerate(c2w):
            m00, m01, m02, m10, m11, m12, m20, m21, m22 = (f64(m[i, j]) for i in range(3) for j in range(3))
            tr = (m00 + m11) + m22
            if tr >= m00 and tr >= m11 and tr >= m22:
                r = np.sqrt(one + tr)
                f = half / r
                q = [r / two, (m21 - m12) * f, (m02 - m20) * f, (m10 - m01) * f]
            elif m00 >= m11 and m00 >= m22:
                r = np.sqrt(((one + m00) - m11) - m22)
                f = half / r
                q = [(m21 - m12) * f, r / two, (m01 + m10) * f, (m02 + m20) * f]
            elif m11 >= m22:
                r = np.sqrt(((one + m11) - m00) - m22)
                f = half / r
                q = [(m02 - m20) * f, (m01 + m10) * f, r / two, (m12 + m21) * f]
            else:
                r = np.sqrt(((one + m22) - m00) - m11)
                f = half / r
                q = [(m10 - m01) * f, (m02 + m20) * f, (m12 + m21) * f, r / two]
            state[v, :4] = normalise(q)
            state[v, 4:] = m[:, 3]
            est[v] = record(state[v], K)
    return state, est


def poses(state):
    """state [V, 7] -> c2w [V, 3, 4] float64"""
    out = np.empty((len(state), 3, 4), np.float64)
    for v, s in enumerate(state):
        out[v, :, :3] = np.array(matrix([f64(c) for c in s[:4]]), np.float64).reshape(3, 3)
        out[v, :, 3] = s[4:]
    return out


def _dot3(a0, b0, a1, b1, a2, b2):
    return (a0 * b0 + a1 * b1) + a2 * b2


def pairs(depth, a, b, M, N, is_disp, near, max_depth, max_dist):
    """one frame: depth [H, W], the estimate's record a [16], the reference record b [16], M [H, W], N [3, H, W] ->
    (pair [H W] bool, J [6][H W] float32, r [H W] float32), pixels in the order i = py W + px"""
    H, W = depth.shape
    near, max_depth, max_dist = f32(near), f32(max_depth), f32(max_dist)
    a = [f32(x) for x in a]
    b = [f32(x) for x in b]
    with np.errstate(all="ignore"):
        d = np.asarray(depth, np.float32).reshape(-1)
        if is_disp:
            d = f32(1) / d
        ok = (d > near) & (d <= max_depth)
        i = np.arange(H * W)
        px, py = (i % W).astype(np.float32), (i // W).astype(np.float32)
        dx, dy = (px - a[14]) / a[12], (py - a[15]) / a[13]
        q0, q1 = dx * d, dy * d
        u = [_dot3(a[3 * k], q0, a[3 * k + 1], q1, a[3 * k + 2], d) for k in range(3)]
        p = [a[9 + k] + u[k] for k in range(3)]
        e = [p[k] - b[9 + k] for k in range(3)]
        xc, yc, zc = (_dot3(b[k], e[0], b[3 + k], e[1], b[6 + k], e[2]) for k in range(3))
        ok &= (zc > near) & (zc > 0)
        ia = (((b[12] * xc) / zc) + b[14]) + f32(0.5)
        ib = (((b[13] * yc) / zc) + b[15]) + f32(0.5)
        ok &= (ia >= 0) & (ia < f32(W)) & (ib >= 0) & (ib < f32(H))
        mx = np.where(ok, ia, f32(0)).astype(np.int32)
        my = np.where(ok, ib, f32(0)).astype(np.int32)
        at = my * W + mx
        s = np.asarray(M, np.float32).reshape(-1)[at]
        ok &= s > 0
        n = [np.asarray(N, np.float32)[k].reshape(-1)[at] for k in range(3)]
        ok &= _dot3(n[0], n[0], n[1], n[1], n[2], n[2]) > 0
        rx, ry = (mx.astype(np.float32) - b[14]) / b[12], (my.astype(np.float32) - b[15]) / b[13]
        delta = []
        for k in range(3):
            w = (b[3 * k] * rx + b[3 * k + 1] * ry) + b[3 * k + 2]
            m = b[9 + k] + s * w
            delta.append(p[k] - m)
        ok &= _dot3(delta[0], delta[0], delta[1], delta[1], delta[2], delta[2]) <= max_dist * max_dist
        ok &= _dot3(n[0], u[0], n[1], u[1], n[2], u[2]) < 0
        r = _dot3(n[0], delta[0], n[1], delta[1], n[2], delta[2])
        J = [n[0], n[1], n[2], u[1] * n[2] - u[2] * n[1], u[2] * n[0] - u[0] * n[2], u[0] * n[1] - u[1] * n[0]]
    assert all(x.dtype == np.float32 for x in J + [r, ia, s] + delta + u)
    return ok, J, r


def sums(ok, J, r):
    """the 29 sums of one frame, in the header's tree -> (S [29] float64, slab [n_groups, 29])"""
    n = len(ok)
    G = -(-n // TILE)
    Jd = [np.where(ok, x, f32(0)).astype(np.float64) for x in J]
    rd = np.where(ok, r, f32(0)).astype(np.float64)
    terms = [Jd[i] * Jd[j] for i, j in PAIRS] + [Jd[i] * rd for i in range(6)] + [rd * rd, ok.astype(np.float64)]
    t = np.zeros((SUMS, G * TILE), np.float64)
    t[:, :n] = np.stack(terms)
    t = t.reshape(SUMS, G, TILE // THREADS, THREADS)
    acc = np.zeros((SUMS, G, THREADS), np.float64)
    for j in range(TILE // THREADS):
        acc = acc + t[:, :, j]
    x = acc.reshape(SUMS, G, THREADS // WAVE, WAVE)
    lane = np.arange(WAVE)
    for mask in (32, 16, 8, 4, 2, 1):
        x = x + x[..., lane ^ mask]
    w = x[..., 0]
    slab = ((w[..., 0] + w[..., 1]) + w[..., 2]) + w[..., 3]      # [29, G]
    S = np.zeros(SUMS, np.float64)
    for g in range(G):
        S = S + slab[:, g]
    return S, slab.T.copy()


def solve(S, min_pairs):
    """-> (status, smallest pivot ratio, x [6] or None)"""
    Hm = np.zeros((6, 6), np.float64)
    for k, (i, j) in enumerate(PAIRS):
        Hm[i, j] = Hm[j, i] = S[k]
    if S[28] < min_pairs:
        return 1, f64(0), None
    top = Hm[0, 0]
    for i in range(1, 6):
        if Hm[i, i] > top:
            top = Hm[i, i]
    if not top > 0:
        return 2, f64(0), None
    floor = f64(PIVOT_EPS) * top
    L = np.zeros((6, 6), np.float64)
    D = np.zeros(6, np.float64)
    ratio = None
    with np.errstate(all="ignore"):
        for j in range(6):
            d = Hm[j, j]
            for k in range(j):
                d = d - (L[j, k] * L[j, k]) * D[k]
            D[j] = d
            rj = d / top
            if ratio is None or rj < ratio:
                ratio = rj
            if not d > floor:
                return 2, ratio, None
            for i in range(j + 1, 6):
                s = Hm[i, j]
                for k in range(j):
                    s = s - (L[i, k] * L[j, k]) * D[k]
                L[i, j] = s / d
        x = np.zeros(6, np.float64)
        for i in range(6):
            y = -S[21 + i]
            for k in range(i):
                y = y - L[i, k] * x[k]
            x[i] = y
        for i in range(6):
            x[i] = x[i] / D[i]
        for i in range(5, -1, -1):
            y = x[i]
            for k in range(i + 1, 6):
                y = y - L[k, i] * x[k]
            x[i] = y
        if not np.isfinite(x).all():
            return 2, ratio, None
    return 0, ratio, x


def update(state, x):
    """the state [7] after the step x = (t, w)"""
    half, one = f64(0.5), f64(1)
    h = [half * x[3], half * x[4], half * x[5]]
    ln = np.sqrt(((one + h[0] * h[0]) + h[1] * h[1]) + h[2] * h[2])
    dw, dx, dy, dz = one / ln, h[0] / ln, h[1] / ln, h[2] / ln
    qw, qx, qy, qz = (f64(c) for c in state[:4])
    q = [((dw * qw - dx * qx) - dy * qy) - dz * qz,
         ((dw * qx + dx * qw) + dy * qz) - dz * qy,
         ((dw * qy - dx * qz) + dy * qw) + dz * qx,
         ((dw * qz + dx * qy) - dy * qx) + dz * qw]
    out = np.empty(7, np.float64)
    out[:4] = normalise(q)
    out[4:] = [state[4] + x[0], state[5] + x[1], state[6] + x[2]]
    return out


def align(depth, guess, K, ref_view, model_depth, model_normal, is_disp=True, near=0.0, max_depth=10.0, iterations=10,
          max_dist=0.3, min_pairs=64):
    """-> dict(state [V, 7] f64, est [V, 16] f32, c2w [V, 3, 4] f64, report [V, iterations, 4] f64, slab [V, n_groups,
    29] f64 of the last iteration)"""
    depth = np.asarray(depth, np.float32)
    V, H, W = depth.shape
    state, est = init(guess, K)
    assert len(state) == V
    ref_view = np.asarray(ref_view, np.float32).reshape(V, 16)
    report = np.zeros((V, iterations, 4), np.float64)
    slabs = [None] * V
    for v in range(V):
        for it in range(iterations):
            ok, J, r = pairs(depth[v], est[v], ref_view[v], model_depth[v], model_normal[v], is_disp, near, max_depth,
                             max_dist)
            S, slabs[v] = sums(ok, J, r)
            status, ratio, x = solve(S, min_pairs)
            report[v, it] = S[28], S[27], status, ratio
            if status == 0:
                state[v] = update(state[v], x)
                est[v] = record(state[v], old=est[v])
    return dict(state=state, est=est, c2w=poses(state), report=report, slab=np.stack(slabs))
