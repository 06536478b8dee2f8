"""include/scsfm_fuse.h restated in numpy: the yardstick of tests/test_fusion_hostsim.py and tests/test_gpu_fusion.py, which
compare the kernels with it bit for bit.  Vectorised over the voxels, one frame after another; every operation is one
numpy operation on np.float32 arrays (numpy neither fuses a multiply with an add nor flushes denormals), the camera
inverse is float64, and there is no cull: every voxel is tested against every frame.  Test infrastructure only."""
from __future__ import annotations

import numpy as np

f32 = np.float32
CHUNK = 1024


def cameras(c2w, K):
    """c2w [n, 12] or [n, 3, 4] float64, K [3, 3] -> [n, 16] float32: the general inverse in the header's order"""
    p = np.asarray(c2w, np.float64).reshape(-1, 3, 4)
    a = [p[:, i // 3, i % 3] for i in range(9)]
    t = [p[:, i, 3] for i in range(3)]
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
    ti = [-((z[3 * i] * t[0] + z[3 * i + 1] * t[1]) + z[3 * i + 2] * t[2]) for i in range(3)]
    K = np.asarray(K, np.float32).reshape(9)
    out = np.empty((len(p), 16), np.float32)
    for i in range(9):
        out[:, i] = z[i].astype(np.float32)
    for i in range(3):
        out[:, 9 + i] = ti[i].astype(np.float32)
    out[:, 12], out[:, 13], out[:, 14], out[:, 15] = K[0], K[4], K[2], K[5]
    return out


def centres(o, n, s):
    return f32(o) + (np.arange(n, dtype=np.float32) + f32(0.5)) * f32(s)


class Volume:
    """the five planes [5, nz, ny, nx] and the header's two operations on them"""

    def __init__(self, dims, origin, voxel_size, trunc=None, max_weight=64.0):
        self.dims = tuple(int(d) for d in dims)
        self.origin = tuple(f32(o) for o in origin)
        self.voxel = f32(voxel_size)
        self.trunc = f32(3 * voxel_size if trunc is None else trunc)
        self.max_weight = f32(max_weight)
        nx, ny, nz = self.dims
        self.planes = np.zeros((5, nz, ny, nx), np.float32)

    tsdf = property(lambda self: self.planes[0])
    weight = property(lambda self: self.planes[1])
    colour = property(lambda self: self.planes[2:])

    def grid(self):
        nx, ny, nz = self.dims
        x = centres(self.origin[0], nx, self.voxel)[None, None, :]
        y = centres(self.origin[1], ny, self.voxel)[None, :, None]
        z = centres(self.origin[2], nz, self.voxel)[:, None, None]
        return x, y, z

    def integrate(self, depth, images, c2w, K, is_disp=True, near=0.0, max_depth=10.0):
        depth = np.asarray(depth, np.float32)
        F, H, W = depth.shape
        cam = cameras(c2w, K)
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
                sdf = d - qz
                ok &= ~(sdf < -self.trunc)
                tn = np.minimum(one, sdf / self.trunc)
                w1 = w + one
                assert all(k.dtype == np.float32 for k in (qx, u, a, d, sdf, tn, w1))
                t[...] = np.where(ok, (t * w + tn) / w1, t)
                if images is not None:
                    for ch in range(3):
                        col = np.asarray(images[f][ch], np.float32)[py, px] * f32(0.225) + f32(0.45)
                        plane = self.planes[2 + ch]
                        plane[...] = np.where(ok, (plane * w + col) / w1, plane)
                w[...] = np.where(ok, np.minimum(w1, self.max_weight), w)

    def crossings(self, min_weight=1.0):
        """the crossings in the header's order -> (a [N] linear index of voxel a, axis [N] 0 / 1 / 2)"""
        nx, ny, nz = self.dims
        t, w = self.planes[0], self.planes[1]
        seen, neg = w >= f32(min_weight), t < 0
        e = np.zeros((nz, ny, nx, 3), bool)
        e[:, :, :-1, 0] = seen[:, :, :-1] & seen[:, :, 1:] & (neg[:, :, :-1] != neg[:, :, 1:])
        e[:, :-1, :, 1] = seen[:, :-1] & seen[:, 1:] & (neg[:, :-1] != neg[:, 1:])
        e[:-1, :, :, 2] = seen[:-1] & seen[1:] & (neg[:-1] != neg[1:])
        flat = np.flatnonzero(e.reshape(-1))  # (voxel-major, then the edge: the header's order)
        return flat // 3, flat % 3

    def count(self, min_weight=1.0):
        return len(self.crossings(min_weight)[0])

    def chunk_counts(self, min_weight=1.0):
        a, _ = self.crossings(min_weight)
        nvox = int(np.prod(self.dims))
        return np.bincount(a // CHUNK, minlength=(nvox + CHUNK - 1) // CHUNK).astype(np.int32)

    def extract(self, min_weight=1.0):
        """-> (xyz float32 [N, 3], rgb uint8 [N, 3], axis [N])"""
        nx, ny, nz = self.dims
        a, axis = self.crossings(min_weight)
        b = a + np.array([1, nx, nx * ny])[axis]
        t = self.planes[0].reshape(-1)
        with np.errstate(all="ignore"):
            frac = t[a] / (t[a] - t[b])
            idx = [a % nx, (a // nx) % ny, a // (nx * ny)]
            xyz = np.empty((len(a), 3), np.float32)
            for k in range(3):
                c = f32(self.origin[k]) + (idx[k].astype(np.float32) + f32(0.5)) * self.voxel
                xyz[:, k] = np.where(axis == k, c + frac * self.voxel, c)
            rgb = np.empty((len(a), 3), np.uint8)
            for ch in range(3):
                col = self.planes[2 + ch].reshape(-1)
                c = col[a] + frac * (col[b] - col[a])
                c = np.where(c >= 0, c, f32(0))
                c = np.where(c <= 1, c, f32(1))
                c = c * f32(255) + f32(0.5)
                assert c.dtype == np.float32 and frac.dtype == np.float32
                rgb[:, ch] = c.astype(np.int32).astype(np.uint8)
        return xyz, rgb, axis
