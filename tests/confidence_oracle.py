"""include/scsfm_conf.h restated in numpy: the yardstick of tests/test_confidence_hostsim.py and tests/test_gpu_confidence.py,
which compare the kernels with it bit for bit.  Vectorised over the pixels (the voxels), one neighbour (one frame) after
another; every operation is one numpy operation on np.float32 arrays (numpy neither fuses a multiply with an add nor
flushes denormals), the pair transforms are float64, and the integration has no cull: every voxel is tested against every
frame.  Test infrastructure only."""
from __future__ import annotations

import numpy as np

import fusion_oracle as FO

f32 = np.float32
MAX_RADIUS = 4
REDUCE = {"mean": 0, "max": 1}


def offsets(radius):
    return list(range(-radius, 0)) + list(range(1, radius + 1))


def pairs(c2w, K, radius):
    """c2w [n, 12] or [n, 3, 4] float64, K [3, 3] -> [n, 2 radius, 16] float32"""
    p = np.asarray(c2w, np.float64).reshape(-1, 3, 4)
    n = len(p)
    K = np.asarray(K, np.float32).reshape(9)
    out = np.zeros((n, 2 * radius, 16), np.float32)
    for i in range(n):
        for s, o in enumerate(offsets(radius)):
            j = i + o
            if j < 0 or j >= n:
                continue
            a = [p[j, k // 3, k % 3] for k in range(9)]
            t = [p[j, k, 3] for k in range(3)]
            b = [p[i, k // 3, k % 3] for k in range(9)]
            u = [p[i, k, 3] for k in range(3)]
            c0, c1, c2 = a[4] * a[8] - a[5] * a[7], a[5] * a[6] - a[3] * a[8], a[3] * a[7] - a[4] * a[6]
            det = (a[0] * c0 + a[1] * c1) + a[2] * c2
            z = [None] * 9
            z[0], z[3], z[6] = c0 / det, c1 / det, c2 / det
            z[1] = (a[2] * a[7] - a[1] * a[8]) / det
            z[4] = (a[0] * a[8] - a[2] * a[6]) / det
            z[7] = (a[1] * a[6] - a[0] * a[7]) / det
            z[2] = (a[1] * a[5] - a[2] * a[4]) / det
            z[5] = (a[2] * a[3] - a[0] * a[5]) / det
            z[8] = (a[0] * a[4] - a[1] * a[3]) / det
            zt = [-((z[3 * r] * t[0] + z[3 * r + 1] * t[1]) + z[3 * r + 2] * t[2]) for r in range(3)]
            for r in range(3):
                for c in range(3):
                    out[i, s, 3 * r + c] = f32((z[3 * r] * b[c] + z[3 * r + 1] * b[3 + c]) + z[3 * r + 2] * b[6 + c])
                out[i, s, 9 + r] = f32(((z[3 * r] * u[0] + z[3 * r + 1] * u[1]) + z[3 * r + 2] * u[2]) + zt[r])
            out[i, s, 12:] = K[0], K[4], K[2], K[5]
    return out


def weights(depth, pair, is_disp=True, max_depth=10.0, min_views=1, floor=0.0, reduce="mean", detail=False):
    """depth [n, H, W], pair [n, 2 radius, 16] -> weight [n, H, W] float32 (with ``detail`` also the counts, int [n, H, W])"""
    depth = np.asarray(depth, np.float32)
    pair = np.asarray(pair, np.float32)
    n, H, W = depth.shape
    radius = pair.shape[1] // 2
    assert pair.shape == (n, 2 * radius, 16) and 1 <= radius <= MAX_RADIUS
    max_depth, floor, one, zero = f32(max_depth), f32(floor), f32(1), f32(0)
    fpx = np.arange(W, dtype=np.float32)[None, :]
    fpy = np.arange(H, dtype=np.float32)[:, None]
    out = np.zeros((n, H, W), np.float32)
    counts = np.zeros((n, H, W), np.int32)
    with np.errstate(all="ignore"):
        inv = one / depth if is_disp else depth
        for i in range(n):
            d = inv[i]
            own = (d > 0) & (d <= max_depth)
            count = np.zeros((H, W), np.int32)
            total = np.zeros((H, W), np.float32)
            best = np.zeros((H, W), np.float32)
            for s, o in enumerate(offsets(radius)):
                c = pair[i, s]
                j = i + o
                if not c[12] > 0 or j < 0 or j >= n:
                    continue
                X = ((fpx - c[14]) / c[12]) * d
                Y = ((fpy - c[15]) / c[13]) * d
                qx = ((c[0] * X + c[1] * Y) + c[2] * d) + c[9]
                qy = ((c[3] * X + c[4] * Y) + c[5] * d) + c[10]
                qz = ((c[6] * X + c[7] * Y) + c[8] * d) + c[11]
                ok = own & (qz > 0)
                u = (c[12] * qx) / qz + c[14]
                v = (c[13] * qy) / qz + c[15]
                g, h = np.floor(u), np.floor(v)
                ok &= (g >= 0) & (g < f32(W)) & (h >= 0) & (h < f32(H))  # (a NaN fails)
                x0 = np.where(ok, g, 0).astype(np.int32)
                y0 = np.where(ok, h, 0).astype(np.int32)
                ok &= (x0 <= W - 2) & (y0 <= H - 2)
                x0, y0 = np.where(ok, x0, 0), np.where(ok, y0, 0)
                x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
                nb = inv[j]
                d00, d01, d10, d11 = nb[y0, x0], nb[y0, x1], nb[y1, x0], nb[y1, x1]
                ok &= (d00 > 0) & (d01 > 0) & (d10 > 0) & (d11 > 0)
                a, b = u - g, v - h
                top = d00 + a * (d01 - d00)
                bot = d10 + a * (d11 - d10)
                p = top + b * (bot - top)
                m = one - np.abs(qz - p) / (qz + p)
                assert all(k.dtype == np.float32 for k in (X, qx, u, g, a, top, p, m))
                count = np.where(ok, count + 1, count)
                total = np.where(ok, total + m, total)
                best = np.where(ok & (m > best), m, best)
            mean = total / np.where(count > 0, count, 1).astype(np.float32)
            c = np.where(count >= min_views, mean if REDUCE[reduce] == 0 else best, zero)
            c = np.where(own & (c >= floor), c, zero)
            assert c.dtype == np.float32
            out[i], counts[i] = c, np.where(own, count, 0)
    return (out, counts) if detail else out


class Volume(FO.Volume):
    """tests/fusion_oracle.py's volume with the header's weighted integration"""

    def integrate(self, depth, images, c2w, K, is_disp=True, near=0.0, max_depth=10.0, weight=None):
        if weight is None:
            return super().integrate(depth, images, c2w, K, is_disp, near, max_depth)
        depth = np.asarray(depth, np.float32)
        weight = np.asarray(weight, np.float32)
        F, H, W = depth.shape
        assert weight.shape == depth.shape
        cam = FO.cameras(c2w, K)
        x, y, z = self.grid()
        near, max_depth, one = f32(near), f32(max_depth), f32(1)
        t, w = self.planes[0], self.planes[1]
        with np.errstate(all="ignore"):
            for f in range(F):
                c = cam[f]
                qx = ((c[0] * x + c[1] * y) + c[2] * z) + c[9]
                qy = ((c[3] * x + c[4] * y) + c[5] * z) + c[10]
                qz = ((c[6] * x + c[7] * y) + c[8] * z) + c[11]
                ok = qz > near
                u = (c[12] * qx) / qz + c[14]
                v = (c[13] * qy) / qz + c[15]
                a, b = u + f32(0.5), v + f32(0.5)
                ok &= (a >= 0) & (a < f32(W)) & (b >= 0) & (b < f32(H))  # (a NaN fails)
                px = np.where(ok, a, 0).astype(np.int32)
                py = np.where(ok, b, 0).astype(np.int32)
                d = depth[f][py, px]
                if is_disp:
                    d = one / d
                ok &= (d > 0) & (d <= max_depth)
                cw = weight[f][py, px]
                ok &= (cw > 0) & (cw <= one)
                sdf = d - qz
                ok &= ~(sdf < -self.trunc)
                tn = np.minimum(one, sdf / self.trunc) * cw
                w1 = w + cw
                assert all(k.dtype == np.float32 for k in (qx, u, a, d, cw, sdf, tn, w1))
                t[...] = np.where(ok, (t * w + tn) / w1, t)
                if images is not None:
                    for ch in range(3):
                        col = (np.asarray(images[f][ch], np.float32)[py, px] * f32(0.225) + f32(0.45)) * cw
                        plane = self.planes[2 + ch]
                        plane[...] = np.where(ok, (plane * w + col) / w1, plane)
                w[...] = np.where(ok, np.minimum(w1, self.max_weight), w)
