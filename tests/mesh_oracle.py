"""include/scsfm_mesh.h restated in numpy: the yardstick of tests/test_mesh_hostsim.py and tests/test_gpu_mesh.py, which
compare the kernels with it bit for bit.  Written from the header's text, not from the kernel's tables: the vertices come
from the crossing rule over the seven edges a voxel owns, the triangles of a tetrahedron from its corners with t < 0 (I)
and the others (O), and a triangle's orientation from an exact integer evaluation with every fraction at one half (the
lattice coordinates doubled).  Every floating-point operation is one numpy operation on np.float32 arrays.  Test
infrastructure only."""
from __future__ import annotations

import numpy as np

f32 = np.float32
# the seven edges voxel a owns, by type e: the offset (dx, dy, dz) of b
EDGES = ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1))
# Kuhn's six tetrahedra round the diagonal 0-7; corner k of a cell is (k & 1, (k >> 1) & 1, k >> 2)
TETS = ((0, 1, 3, 7), (0, 1, 5, 7), (0, 2, 3, 7), (0, 2, 6, 7), (0, 4, 5, 7), (0, 4, 6, 7))


def corner(k):
    return np.array([k & 1, (k >> 1) & 1, k >> 2])


def case_triangles(tet, inside):
    """The triangles of tetrahedron ``tet`` (a corner list) whose corners with t < 0 are ``inside`` (a set): a list of
    triangles, each three edges (p, q) of cell corners with p the edge's owner, in the header's order and orientation."""
    I = [c for c in tet if c in inside]
    O = [c for c in tet if c not in inside]
    if len(I) == 1:
        tris = [[(I[0], O[0]), (I[0], O[1]), (I[0], O[2])]]
    elif len(I) == 3:
        tris = [[(I[0], O[0]), (I[1], O[0]), (I[2], O[0])]]
    elif len(I) == 2:
        q = [(I[0], O[0]), (I[0], O[1]), (I[1], O[1]), (I[1], O[0])]
        tris = [[q[0], q[1], q[2]], [q[0], q[2], q[3]]]
    else:
        return []
    # counter-clockwise seen from the O side: (B - A) x (C - A) points from the I corners to the O corners.  Every
    # fraction one half, coordinates doubled: a vertex is the sum of its edge's two corners, all integers.
    towards = len(I) * sum(corner(c) for c in O) - len(O) * sum(corner(c) for c in I)
    out = []
    for tri in tris:
        A, B, C = (corner(p) + corner(q) for p, q in tri)
        s = int(np.dot(np.cross(B - A, C - A), towards))
        assert s != 0
        if s < 0:
            tri = [tri[0], tri[2], tri[1]]
        out.append([(min(p, q), max(p, q)) for p, q in tri])
    return out


def centres(o, n, s):
    return f32(o) + (np.arange(n, dtype=np.float32) + f32(0.5)) * f32(s)


def mesh(planes, origin, voxel, min_weight=1.0):
    """planes [5, nz, ny, nx] float32 -> dict(xyz float32 [V, 3], rgb uint8 [V, 3], tri int32 [T, 3], a [V] the owning
    voxel of every vertex, e [V] its edge type, cases int [6, 16] how many seen tetrahedra of each kind had each 4-bit
    case (bit j: corner j of the tetrahedron's list has t < 0))"""
    planes = np.asarray(planes, np.float32)
    _, nz, ny, nx = planes.shape
    voxel = f32(voxel)
    t, w = planes[0], planes[1]
    seen, neg = w >= f32(min_weight), t < 0
    cross = np.zeros((nz, ny, nx, 7), bool)
    for e, (dx, dy, dz) in enumerate(EDGES):
        if nx - dx <= 0 or ny - dy <= 0 or nz - dz <= 0:
            continue
        sa = (slice(0, nz - dz), slice(0, ny - dy), slice(0, nx - dx))
        sb = (slice(dz, nz), slice(dy, ny), slice(dx, nx))
        cross[sa + (e,)] = seen[sa] & seen[sb] & (neg[sa] != neg[sb])
    flat = np.flatnonzero(cross.reshape(-1))  # (voxel-major, then the edge type: the header's order)
    a, e = flat // 7, flat % 7
    offs = np.array(EDGES)
    step = offs @ np.array([1, nx, nx * ny])
    b = a + step[e]
    tf = t.reshape(-1)
    with np.errstate(all="ignore"):
        frac = tf[a] / (tf[a] - tf[b])
        idx = [a % nx, (a // nx) % ny, a // (nx * ny)]
        xyz = np.empty((len(a), 3), np.float32)
        for k in range(3):
            c = f32(origin[k]) + (idx[k].astype(np.float32) + f32(0.5)) * voxel
            xyz[:, k] = np.where(offs[e, k] == 1, c + frac * voxel, c)
        xyz[np.isnan(xyz)] = f32(np.nan)  # (a NaN coordinate is the quiet NaN 0x7fc00000)
        assert (xyz.view(np.uint32)[np.isnan(xyz)] == 0x7fc00000).all()
        rgb = np.empty((len(a), 3), np.uint8)
        for ch in range(3):
            col = planes[2 + ch].reshape(-1)
            c = col[a] + frac * (col[b] - col[a])
            c = np.where(c >= 0, c, f32(0))
            c = np.where(c <= 1, c, f32(1))
            c = c * f32(255) + f32(0.5)
            assert c.dtype == np.float32 and frac.dtype == np.float32
            rgb[:, ch] = c.astype(np.int32).astype(np.uint8)
    vid = np.full(nz * ny * nx * 7, -1, np.int64)
    vid[flat] = np.arange(len(flat))

    cases = np.zeros((6, 16), np.int64)
    rows = []  # (cell, tetrahedron, first / second triangle, i0, i1, i2)
    if nx > 1 and ny > 1 and nz > 1:
        cz, cy, cx = np.meshgrid(np.arange(nz - 1), np.arange(ny - 1), np.arange(nx - 1), indexing="ij")
        cell = ((cz * ny + cy) * nx + cx).reshape(-1)
        lin = lambda k: cell + (k & 1) + ((k >> 1) & 1) * nx + (k >> 2) * nx * ny  # noqa: E731
        sf, nf = seen.reshape(-1), neg.reshape(-1)
        for ti, tet in enumerate(TETS):
            ok = np.logical_and.reduce([sf[lin(k)] for k in tet])
            code = sum(nf[lin(k)].astype(np.int64) << j for j, k in enumerate(tet))
            cases[ti] = np.bincount(code[ok], minlength=16)
            for c4 in range(1, 15):
                at = cell[ok & (code == c4)]
                if not len(at):
                    continue
                inside = {k for j, k in enumerate(tet) if (c4 >> j) & 1}
                for j, tri in enumerate(case_triangles(tet, inside)):
                    ids = []
                    for p, q in tri:
                        d = corner(q) - corner(p)
                        assert d.min() >= 0 and d.max() == 1  # (the owner is the lower corner)
                        v = vid[(at + int(corner(p) @ np.array([1, nx, nx * ny]))) * 7 + EDGES.index(tuple(d))]
                        assert (v >= 0).all()  # (an edge of a seen tetrahedron with a sign change is a crossing)
                        ids.append(v)
                    rows.append(np.stack([at, np.full_like(at, ti), np.full_like(at, j), *ids], axis=1))
    if rows:
        rows = np.concatenate(rows)
        rows = rows[np.lexsort((rows[:, 2], rows[:, 1], rows[:, 0]))]
        tri = rows[:, 3:].astype(np.int32)
    else:
        tri = np.zeros((0, 3), np.int32)
    return dict(xyz=xyz, rgb=rgb, tri=np.ascontiguousarray(tri), a=a, e=e, cases=cases)
