"""include/scsfm_cast.h restated in numpy: the yardstick of tests/test_raycast_hostsim.py and tests/test_gpu_raycast.py,
which compare the kernels with it bit for bit.  Vectorised over the pixels of all views, one sample after another; every
operation is one numpy operation on np.float32 arrays (numpy neither fuses a multiply with an add nor flushes denormals,
and its division and square root are correctly rounded).  There is no cull: every sample of every ray is evaluated, with
its gradient and colours, until the ray's event.  Test infrastructure only."""
from __future__ import annotations

import numpy as np

f32 = np.float32
QNAN = np.frombuffer(np.uint32(0x7fc00000).tobytes(), np.float32)[0]


def views(c2w, K):
    """c2w [n, 12] or [n, 3, 4] float64, K [3, 3] -> [n, 16] float32: A row-major, the centre, fx fy cx cy"""
    p = np.asarray(c2w, np.float64).reshape(-1, 3, 4)
    K = np.asarray(K, np.float32).reshape(9)
    out = np.empty((len(p), 16), np.float32)
    out[:, :9] = p[:, :, :3].reshape(-1, 9).astype(np.float32)
    out[:, 9:12] = p[:, :, 3].astype(np.float32)
    out[:, 12], out[:, 13], out[:, 14], out[:, 15] = K[0], K[4], K[2], K[5]
    return out


def brick_mask(planes, min_weight=1.0):
    """one byte per brick of 8 x 8 x 8 voxels, x fastest: some voxel of its nine-wide (clipped) range is seen and < 0"""
    t, w = planes[0], planes[1]
    nz, ny, nx = t.shape
    neg = (w >= f32(min_weight)) & (t < 0)
    nb = [-(-n // 8) for n in (nx, ny, nz)]
    out = np.zeros((nb[2], nb[1], nb[0]), np.uint8)
    for bz in range(nb[2]):
        for by in range(nb[1]):
            for bx in range(nb[0]):
                out[bz, by, bx] = neg[8 * bz:8 * bz + 9, 8 * by:8 * by + 9, 8 * bx:8 * bx + 9].any()
    return out.reshape(-1)


def lerp(a, b, f):
    return a + f * (b - a)


def rays(view, hw):
    """-> (c [3][V, 1, 1], w [3][V, H, W]) float32"""
    H, W = hw
    view = np.asarray(view, np.float32)
    a = [view[:, i][:, None, None] for i in range(16)]
    px = np.arange(W, dtype=np.float32)[None, None, :]
    py = np.arange(H, dtype=np.float32)[None, :, None]
    with np.errstate(all="ignore"):
        dx = (px - a[14]) / a[12]
        dy = (py - a[15]) / a[13]
        w = [np.broadcast_to((a[3 * i] * dx + a[3 * i + 1] * dy) + a[3 * i + 2], (len(view), H, W)) for i in range(3)]
    assert all(k.dtype == np.float32 for k in w)
    return [a[9], a[10], a[11]], w


def field(planes, origin, voxel, p, min_weight):
    """the field at the points p (three float32 arrays of one shape) -> (valid, T, G [3], C [3]); T, G and C are 0 where
    the sample is not valid"""
    _, nz, ny, nx = planes.shape
    shape = p[0].shape
    with np.errstate(all="ignore"):
        g = [((p[i] - f32(origin[i])) / f32(voxel)) - f32(0.5) for i in range(3)]
        inr = np.ones(shape, bool)
        for gi, n in zip(g, (nx, ny, nz)):
            inr &= (gi >= 0) & (gi < f32(n - 1))  # (a NaN fails)
    sel = np.flatnonzero(inr.reshape(-1))
    valid = np.zeros(shape, bool)
    T = np.zeros(shape, np.float32)
    G = [np.zeros(shape, np.float32) for _ in range(3)]
    C = [np.zeros(shape, np.float32) for _ in range(3)]
    if not len(sel):
        return valid, T, G, C
    gs = [gi.reshape(-1)[sel] for gi in g]
    b = [gi.astype(np.int32) for gi in gs]
    fx, fy, fz = (gi - bi.astype(np.float32) for gi, bi in zip(gs, b))
    base = (b[2].astype(np.int64) * ny + b[1]) * nx + b[0]
    offs = [i + nx * j + nx * ny * k for k in (0, 1) for j in (0, 1) for i in (0, 1)]   # q[i + 2 j + 4 k]

    def corners(plane):
        flat = plane.reshape(-1)
        return [flat[base + o] for o in offs]

    def tri(q):
        e00, e10 = lerp(q[0], q[1], fx), lerp(q[2], q[3], fx)
        e01, e11 = lerp(q[4], q[5], fx), lerp(q[6], q[7], fx)
        return lerp(lerp(e00, e10, fy), lerp(e01, e11, fy), fz)

    with np.errstate(all="ignore"):
        ok = np.logical_and.reduce([q >= f32(min_weight) for q in corners(planes[1])])
        q = corners(planes[0])
        t = tri(q)
        gx = lerp(lerp(q[1] - q[0], q[3] - q[2], fy), lerp(q[5] - q[4], q[7] - q[6], fy), fz)
        gy = lerp(lerp(q[2] - q[0], q[3] - q[1], fx), lerp(q[6] - q[4], q[7] - q[5], fx), fz)
        gz = lerp(lerp(q[4] - q[0], q[5] - q[1], fx), lerp(q[6] - q[2], q[7] - q[3], fx), fy)
        cols = [tri(corners(planes[2 + ch])) for ch in range(3)]
    assert all(k.dtype == np.float32 for k in (t, gx, gy, gz, fx, *cols))
    keep = sel[ok]
    valid.reshape(-1)[keep] = True
    T.reshape(-1)[keep] = t[ok]
    for dst, src in zip(G + C, [gx, gy, gz] + cols):
        dst.reshape(-1)[keep] = src[ok]
    return valid, T, G, C


def unit_byte(c):
    with np.errstate(all="ignore"):
        c = np.where(c >= 0, c, f32(0))
        c = np.where(c <= 1, c, f32(1))
        c = c * f32(255) + f32(0.5)
    assert c.dtype == np.float32
    return c.astype(np.int32).astype(np.uint8)


def quiet(x):
    return np.where(np.isnan(x), QNAN, x).astype(np.float32)


def cast(planes, origin, voxel, view, hw, near, step, n_steps, min_weight=1.0):
    """-> dict(depth [V, H, W] f32, normal [V, 3, H, W] f32, rgb [V, H, W, 3] u8, shade [V, H, W] u8, hit [V, H, W] bool,
    back [V, H, W] bool: the rays that ended on the back-face rule)"""
    planes = np.asarray(planes, np.float32)
    H, W = hw
    c, w = rays(view, hw)
    V = len(np.asarray(view))
    shape = (V, H, W)
    near, step = f32(near), f32(step)
    done = np.zeros(shape, bool)
    hit = np.zeros(shape, bool)
    back = np.zeros(shape, bool)
    depth = np.zeros(shape, np.float32)
    normal = np.zeros((V, 3, H, W), np.float32)
    rgb = np.zeros((V, H, W, 3), np.uint8)
    shade = np.zeros(shape, np.uint8)
    prev = None
    s_prev = None
    with np.errstate(all="ignore"):
        wl = np.sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2])
        for k in range(int(n_steps)):
            s = near + f32(k) * step
            assert s.dtype == np.float32
            cur = field(planes, origin, voxel, [c[i] + s * w[i] for i in range(3)], min_weight)
            if prev is not None:
                (v0, T0, G0, C0), (v1, T1, G1, C1) = prev, cur
                event = ~done & v0 & v1 & ((T0 < 0) != (T1 < 0))
                h = event & (T1 < 0)
                back |= event & ~h
                done |= event
                if h.any():
                    hit |= h
                    frac = T0 / (T0 - T1)
                    d = quiet(s_prev + (s - s_prev) * frac)
                    depth[h] = d[h]
                    N = [lerp(G0[i], G1[i], frac) for i in range(3)]
                    ln = np.sqrt((N[0] * N[0] + N[1] * N[1]) + N[2] * N[2])
                    n = [np.where(ln > 0, quiet(N[i] / ln), f32(0)) for i in range(3)]
                    for i in range(3):
                        normal[:, i][h] = n[i][h]
                    L = -((n[0] * w[0] + n[1] * w[1]) + n[2] * w[2]) / wl
                    assert L.dtype == np.float32 and frac.dtype == np.float32 and d.dtype == np.float32
                    shade[h] = unit_byte(L)[h]
                    for ch in range(3):
                        rgb[..., ch][h] = unit_byte(lerp(C0[ch], C1[ch], frac))[h]
            prev, s_prev = cur, s
    return dict(depth=depth, normal=normal, rgb=rgb, shade=shade, hit=hit, back=back)
