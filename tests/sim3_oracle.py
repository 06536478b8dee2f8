"""include/scsfm_sim3.h restated in numpy: the yardstick of tests/test_similarity_hostsim.py and
tests/test_gpu_similarity.py, which compare the kernels with it bit for bit.  As tests/track_oracle.py: the pair of a pixel
is one numpy operation on np.float32 arrays per operation of the header, the 37 sums are np.float64 arrays added in the
header's tree, the solve is scalar np.float64.  The quaternion, its matrix, the record and the pose update are
track_oracle's own functions (the two headers state the same rule for them); the pair, the sums, the solve and the scale
are restated here.  It takes the inputs of scsfm_hip.similarity.align.  Test infrastructure only."""
from __future__ import annotations

import numpy as np

import track_oracle as TO

f32 = np.float32
f64 = np.float64
TILE, THREADS, WAVE, SUMS, STATE, REPORT = 1024, 256, 64, 37, 8, 6
PIVOT_EPS = 1e-8
MIN_SCALE_PIVOT = 2e-3
PAIRS = [(i, j) for i in range(7) for j in range(i, 7)]
_dot3 = TO._dot3


def init(c2w, scale0, K):
    """c2w [V, 12] or [V, 3, 4] float64, scale0 [V] float64 -> (state [V, 8] float64, est [V, 16] float32, sigma_f [V]
    float32)"""
    pose, est = TO.init(c2w, K)
    scale0 = np.asarray(scale0, np.float64).reshape(len(pose))
    state = np.concatenate([pose, scale0[:, None]], axis=1)
    with np.errstate(all="ignore"):      # (a scale beyond fp32's range becomes an infinity, as on the device)
        return state, est, scale0.astype(np.float32)


def poses(state):
    """state [V, 8] -> (c2w [V, 3, 4] float64, scale [V] float64)"""
    return TO.poses(state[:, :7]), state[:, 7].copy()


def scaled_depth(depth, sigma_f, is_disp):
    """depth [V, H, W] float32, sigma_f [V] float32 -> fl(sigma_f d0) [V, H, W] float32: the depth the tracker sees"""
    with np.errstate(all="ignore"):
        d = np.asarray(depth, np.float32)
        if is_disp:
            d = f32(1) / d
        out = np.asarray(sigma_f, np.float32).reshape(-1, 1, 1) * d
    assert out.dtype == np.float32
    return out


def pairs(depth, sigma_f, a, b, M, N, is_disp, near, max_depth, max_dist):
    """one frame: depth [H, W], the frame's fp32 scale, the estimate's record a [16], the reference record b [16], M
    [H, W], N [3, H, W] -> (pair [H W] bool, J [7][H W] float32, r [H W] float32), pixels in the order i = py W + px"""
    H, W = depth.shape
    near, max_depth, max_dist = f32(near), f32(max_depth), f32(max_dist)
    a = [f32(x) for x in a]
    b = [f32(x) for x in b]
    with np.errstate(all="ignore"):
        d = np.asarray(depth, np.float32).reshape(-1)
        if is_disp:
            d = f32(1) / d
        d = f32(sigma_f) * d
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
        nu = _dot3(n[0], u[0], n[1], u[1], n[2], u[2])
        ok &= nu < 0
        r = _dot3(n[0], delta[0], n[1], delta[1], n[2], delta[2])
        J = [n[0], n[1], n[2], u[1] * n[2] - u[2] * n[1], u[2] * n[0] - u[0] * n[2], u[0] * n[1] - u[1] * n[0], nu]
    assert all(x.dtype == np.float32 for x in J + [r, ia, s, d] + delta + u)
    return ok, J, r


def sums(ok, J, r):
    """the 37 sums of one frame, in the header's tree -> (S [37] float64, slab [n_groups, 37])"""
    n = len(ok)
    G = -(-n // TILE)
    Jd = [np.where(ok, x, f32(0)).astype(np.float64) for x in J]
    rd = np.where(ok, r, f32(0)).astype(np.float64)
    terms = [Jd[i] * Jd[j] for i, j in PAIRS] + [Jd[i] * rd for i in range(7)] + [rd * rd, ok.astype(np.float64)]
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
    slab = ((w[..., 0] + w[..., 1]) + w[..., 2]) + w[..., 3]      # [37, G]
    S = np.zeros(SUMS, np.float64)
    for g in range(G):
        S = S + slab[:, g]
    return S, slab.T.copy()


def solve(S, sigma, min_pairs, min_scale_pivot):
    """-> (status, smallest ratio of pivots 0 .. 5, ratio of pivot 6, x [7] or None); status 3: x[6] is 0"""
    zero = f64(0)
    sigma = f64(sigma)
    with np.errstate(all="ignore"):
        if not (sigma > 0 and sigma - sigma == 0):
            return 2, zero, zero, None
    if S[36] < min_pairs:
        return 1, zero, zero, None
    Hm = np.zeros((7, 7), np.float64)
    for k, (i, j) in enumerate(PAIRS):
        Hm[i, j] = Hm[j, i] = S[k]
    top6 = Hm[0, 0]
    for i in range(1, 6):
        if Hm[i, i] > top6:
            top6 = Hm[i, i]
    if not top6 > 0:
        return 2, zero, zero, None
    top = Hm[6, 6] if Hm[6, 6] > top6 else top6
    floor = f64(PIVOT_EPS) * top6
    L = np.zeros((7, 7), np.float64)
    D = np.zeros(7, np.float64)
    ratio = None
    with np.errstate(all="ignore"):
        for j in range(6):
            d = Hm[j, j]
            for k in range(j):
                d = d - (L[j, k] * L[j, k]) * D[k]
            D[j] = d
            rj = d / top6
            if ratio is None or rj < ratio:
                ratio = rj
            if not d > floor:
                return 2, ratio, zero, None
            for i in range(j + 1, 7):
                s = Hm[i, j]
                for k in range(j):
                    s = s - (L[i, k] * L[j, k]) * D[k]
                L[i, j] = s / d
        d = Hm[6, 6]
        for k in range(6):
            d = d - (L[6, k] * L[6, k]) * D[k]
        D[6] = d
        ratio6 = d / top
        held = not d > f64(min_scale_pivot) * top
        z = np.zeros(7, np.float64)
        for i in range(7):
            y = -S[28 + i]
            for k in range(i):
                y = y - L[i, k] * z[k]
            z[i] = y
        for i in range(7):
            z[i] = z[i] / D[i]
        if not held and not (z[6] > -1 and z[6] < 1):
            held = True
        x = np.zeros(7, np.float64)
        x[6] = zero if held else z[6]
        for i in range(5, -1, -1):
            y = z[i]
            for k in range(i + 1, 6):
                y = y - L[k, i] * x[k]
            if not held:
                y = y - L[6, i] * x[6]
            x[i] = y
        if not np.isfinite(x).all():
            return 2, ratio, ratio6, None
    return (3 if held else 0), ratio, ratio6, x


def update(state, x, status):
    """the state [8] after the step x = (t, w, lambda)"""
    out = np.empty(8, np.float64)
    out[:7] = TO.update(state[:7], x[:6])
    sigma = f64(state[7])
    if status == 0:
        half, one = f64(0.5), f64(1)
        h = half * x[6]
        sigma = (sigma * (one + h)) / (one - h)
    out[7] = sigma
    return out


def align(depth, guess, scale0, K, ref_view, model_depth, model_normal, is_disp=True, near=0.0, max_depth=10.0,
          iterations=10, max_dist=0.3, min_pairs=64, min_scale_pivot=MIN_SCALE_PIVOT):
    """-> dict(state [V, 8] f64, est [V, 16] f32, sigma_f [V] f32, c2w [V, 3, 4] f64, scale [V] f64, report [V,
    iterations, 6] f64, slab [V, n_groups, 37] f64 of the last iteration)"""
    depth = np.asarray(depth, np.float32)
    V, H, W = depth.shape
    state, est, sigma_f = init(guess, scale0, K)
    assert len(state) == V
    ref_view = np.asarray(ref_view, np.float32).reshape(V, 16)
    report = np.zeros((V, iterations, REPORT), np.float64)
    slabs = [None] * V
    for v in range(V):
        for it in range(iterations):
            ok, J, r = pairs(depth[v], sigma_f[v], est[v], ref_view[v], model_depth[v], model_normal[v], is_disp, near,
                             max_depth, max_dist)
            S, slabs[v] = sums(ok, J, r)
            status, ratio, ratio6, x = solve(S, state[v, 7], min_pairs, min_scale_pivot)
            report[v, it] = S[36], S[35], status, ratio, ratio6, state[v, 7]
            if status in (0, 3):
                state[v] = update(state[v], x, status)
                est[v] = TO.record(state[v, :7], old=est[v])
                if status == 0:
                    with np.errstate(all="ignore"):
                        sigma_f[v] = np.float32(state[v, 7])
    c2w, scale = poses(state)
    return dict(state=state, est=est, sigma_f=sigma_f, c2w=c2w, scale=scale, report=report, slab=np.stack(slabs))
