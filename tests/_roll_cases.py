"""The cases tests/test_rolling_hostsim.py (host simulator) and tests/test_gpu_rolling.py (device) both run, each against
tests/rolling_oracle.py bit for bit: the shift of the five planes, the extraction of the crossings that leave, the partition
of a volume's crossings by a keep box, and a window that moves along a drive against one big volume on the same lattice.

A backend has `shift(planes, s, lead=0) -> dst` (dst pre-filled with NaN between guards, src compared after the call),
`leaving(planes, dims, origin, voxel, box, min_weight, capacity=None) -> (count, workspace, xyz, rgb)`,
`rolling(dims, origin0, voxel, frames_per_launch)` -- an object with scsfm_hip.rolling.RollingVolume's shift / integrate /
extract / offset --, `shift_for`, and `dev` / `host` to move arrays.  References are computed once and shared, read-only.
Test infrastructure only."""
from __future__ import annotations

import functools

import numpy as np

import _fusion_cases as F
import fusion_oracle as O
import rolling_oracle as RO

f32 = np.float32
DIMS = F.DIMS                      # (37, 18, 29): x no multiple of 4 or of the 32-wide tile, 19314 voxels a plane (2 mod 4)
SMALL = ((4, 1, 1), (1, 1, 1))
same_bits = F.same_bits


@functools.lru_cache(maxsize=None)
def patterns(dims):
    """[5, nz, ny, nx] float32 whose elements all have distinct bits, NaNs (quiet, signalling, negative), infinities,
    denormals and both zeros among them; none has the bits of numpy's NaN, which dst is pre-filled with"""
    nx, ny, nz = dims
    n = 5 * nx * ny * nz
    bits = ((np.arange(n, dtype=np.uint64) * 2654435761 + 12345) % 2 ** 32).astype(np.uint32)
    special = np.array([0x7FC00001, 0x7F800001, 0xFFC12345, 0x7F800000, 0xFF800000, 0x00000001, 0x807FFFFF, 0x80000000,
                        0x00000000, 0x7FFFFFFF], np.uint32)[:n]
    bits[np.isin(bits, special)] ^= 0x00100000
    at = np.linspace(0, n - 1, len(special)).astype(int)       # (first and last element included)
    bits[at] = special
    assert len(np.unique(bits)) == n and not (bits == 0x7FC00000).any()
    out = bits.view(np.float32).reshape(5, nz, ny, nx)
    out.setflags(write=False)
    return out


def shifts(dims=DIMS):
    out = [(0, 0, 0)]
    for axis in range(3):
        for k in (1, -1, 3, -5, 8, -8):
            out.append(tuple(k if a == axis else 0 for a in range(3)))
    out += [(8, -8, 16), (-3, 5, -7)]
    for axis in range(3):
        n = dims[axis]
        for k in (n - 1, n, -(n + 3)):
            out.append(tuple(k if a == axis else 0 for a in range(3)))
    return out


SMALL_SHIFTS = {(4, 1, 1): [(0, 0, 0), (1, 0, 0), (-1, 0, 0), (3, 0, 0), (4, 0, 0), (-7, 0, 0), (0, 1, 0), (0, 0, -1)],
                (1, 1, 1): [(0, 0, 0), (1, 0, 0), (0, -1, 0), (0, 0, 1)]}
SHIFT_CASES = [(DIMS, s) for s in shifts()] + [(d, s) for d in SMALL for s in SMALL_SHIFTS[d]]


def shift_id(case):
    return "{}x{}x{}:{},{},{}".format(*case[0], *case[1])


def check_shift(case, backend):
    """every element of dst, by bits; with dst on a 16-byte boundary and 1, 2 and 3 floats past one"""
    dims, s = case
    src = patterns(dims)
    want = RO.shift_planes(src, s)
    for lead in (0, 1, 2, 3):
        got = backend.shift(src, s, lead=lead)
        assert same_bits(got.view(np.uint32), want.view(np.uint32)), (dims, s, lead)
    return want


# ---- the leaving extraction ----

VOLUMES = ("straddle_F5", "inside", "dirty_depth")
MIN_WEIGHTS = (1.0, 2.0)


def boxes(dims=DIMS):
    nx, ny, nz = dims
    out = {"empty": (0, 0, 0, 0, 0, 0), "empty_x": (9, 9, 0, ny, 0, nz), "empty_z": (0, nx, 0, ny, 20, 3),
           "whole": (0, nx, 0, ny, 0, nz), "beyond": (-5, nx + 5, -1, ny + 1, -9, nz + 9)}
    for s in ((8, 0, 0), (0, -8, 0), (0, 0, 8), (-3, 5, -7)):
        out["shift_{}_{}_{}".format(*s)] = RO.keep_box(dims, s)
    out["one_thick_x"] = (17, 18, 0, ny, 0, nz)
    out["one_thick_z"] = (0, nx, 0, ny, 11, 12)
    out["cuts_a_chunk"] = (5, 30, 3, 14, 2, 20)       # a chunk is 1024 voxels: 27.7 rows, 1.54 slices
    return out


BOX_NAMES = tuple(boxes())
LEAVING_CASES = [(v, w, b) for v in VOLUMES for w in MIN_WEIGHTS for b in BOX_NAMES]


@functools.lru_cache(maxsize=None)
def leaving_reference(name, min_weight, box_name):
    vol = F.reference(name)[0]
    xyz, rgb, counts = RO.leaving(vol, boxes(vol.dims)[box_name], min_weight)
    for a in (xyz, rgb, counts):
        a.setflags(write=False)
    return xyz, rgb, counts


def check_leaving(case, backend):
    """the count, the workspace, the points and colours in order, at capacity == total and at a smaller one"""
    name, min_weight, box_name = case
    vol = F.reference(name)[0]
    box = boxes(vol.dims)[box_name]
    xyz, rgb, counts = leaving_reference(*case)
    total, ws, got_xyz, got_rgb = backend.leaving(vol.planes, vol.dims, vol.origin, vol.voxel, box, min_weight)
    nc = len(counts)
    assert total == len(xyz) and ws[0] == total, (case, total, len(xyz))
    assert np.array_equal(ws[4:4 + nc], counts), case
    assert np.array_equal(ws[4 + nc:4 + 2 * nc], np.cumsum(counts) - counts), case
    assert same_bits(got_xyz, xyz) and same_bits(got_rgb, rgb), case
    if box_name.startswith("empty"):
        full_xyz, full_rgb, _ = vol.extract(min_weight)
        assert same_bits(got_xyz, full_xyz) and same_bits(got_rgb, full_rgb), case
        assert total > 40 or min_weight > 1, case
    if box_name in ("whole", "beyond"):
        assert total == 0 and not ws[4:4 + 2 * nc].any(), case
    if total > 1:
        cap = max(1, total - 37)
        _, _, part_xyz, part_rgb = backend.leaving(vol.planes, vol.dims, vol.origin, vol.voxel, box, min_weight, cap)
        assert same_bits(part_xyz, xyz[:cap]) and same_bits(part_rgb, rgb[:cap]), (case, cap)
    return total


def rows(xyz, rgb):
    """one record of 15 bytes per point: the bits of xyz and the colour"""
    rec = np.empty(len(xyz), dtype=[("xyz", "<u4", 3), ("rgb", "u1", 3)])
    rec["xyz"], rec["rgb"] = np.ascontiguousarray(xyz, np.float32).view(np.uint32), rgb
    return sorted(r.tobytes() for r in rec)


def check_partition(s, backend, name="straddle_F5", min_weight=1.0):
    """the points emitted with the keep box of the shift s, together with the crossings the oracle finds with both ends
    inside it, are the full extraction as a multiset, with no row twice"""
    vol = F.reference(name)[0]
    box = RO.keep_box(vol.dims, s)
    full_xyz, full_rgb, _ = vol.extract(min_weight)
    stay = ~RO.leaves(vol, box, min_weight)
    _, _, xyz, rgb = backend.leaving(vol.planes, vol.dims, vol.origin, vol.voxel, box, min_weight)
    both = rows(xyz, rgb) + rows(full_xyz[stay], full_rgb[stay])
    assert len(xyz) + int(stay.sum()) == len(full_xyz), s
    assert sorted(both) == rows(full_xyz, full_rgb) and len(set(both)) == len(both), s
    return len(xyz)


# ---- the moving window against one big volume ----

DRIVE = dict(voxel=0.125, origin0=(-2.5, -1.0, -3.0), window=(40, 16, 48), step=8, big=(56, 16, 112), frames=80,
             near=0.05, max_depth=1.5, min_weight=1.0, shifts=10, offset=(16, 0, 64), streamed=519, final=708)
DRIVE_K = np.array([[12.0, 0, 9.5], [0, 12.0, 5.5], [0, 0, 1]], np.float32)
DRIVE_HW = (12, 20)


@functools.lru_cache(maxsize=1)
def drive():
    """80 frames with identity rotation at (0.03 k, 0, 0.11 k) that see the floor y = 0.6 with 1 % noise, random images"""
    n, (H, W) = DRIVE["frames"], DRIVE_HW
    rng = np.random.default_rng(0)
    c2w = np.stack([np.concatenate([np.eye(3), [[0.03 * k], [0.0], [0.11 * k]]], axis=1) for k in range(n)])
    ry = np.broadcast_to(((np.arange(H) - DRIVE_K[1, 2]) / DRIVE_K[1, 1])[:, None], (H, W))
    with np.errstate(all="ignore"):
        floor = np.where(ry > 0, 0.6 / ry, 0.0)
    depth = (floor[None] * (1 + 0.01 * rng.standard_normal((n, H, W)))).astype(np.float32)
    images = rng.standard_normal((n, 3, H, W)).astype(np.float32)
    for a in (c2w, depth, images):
        a.setflags(write=False)
    return dict(c2w=c2w, depth=depth, images=images)


def run_drive(volume, shift_for, dev, host, frames_per_launch):
    """-> (the shifts [(frame, s, xyz, rgb)], the final (xyz, rgb), the volume).  The window is placed from every frame's
    centre before the frame is fused; the frames between two moves go into the volume in calls of at most
    ``frames_per_launch``, which leaves the bits of one call per frame (include/scsfm_fuse.h)."""
    d, D = drive(), DRIVE
    K = dev(DRIVE_K)
    events, pending = [], []

    def flush():
        if pending:
            a, b = pending[0], pending[-1] + 1
            volume.integrate(dev(d["depth"][a:b]), dev(d["images"][a:b]), dev(d["c2w"][a:b]), K, is_disp=False,
                             near=D["near"], max_depth=D["max_depth"])
            del pending[:]

    for k in range(D["frames"]):
        s = shift_for(d["c2w"][k][:, 3], volume.origin0, volume.offset, volume.dims, volume.voxel, D["step"])
        if any(s):
            flush()
            xyz, rgb = volume.shift(s, D["min_weight"])
            events.append((k, tuple(s), host(xyz), host(rgb)))
        pending.append(k)
        if len(pending) == frames_per_launch:
            flush()
    flush()
    xyz, rgb = volume.extract(D["min_weight"])[:2]
    return events, (host(xyz), host(rgb)), volume


@functools.lru_cache(maxsize=1)
def drive_reference():
    """the oracle's rolled run, with the issue's conditions: 10 shifts to the offset (16, 0, 64), 519 points streamed out
    and 708 at the end, and its 1227 rows, sorted, equal the sorted extraction of one 56 x 16 x 112 volume at origin0 fused
    with the same 80 frames"""
    d, D = drive(), DRIVE
    vol = RO.RollingVolume(D["window"], D["origin0"], D["voxel"])
    events, final, _ = run_drive(vol, RO.shift_for, lambda a: a, lambda a: a, 1)
    assert len(events) == D["shifts"] and vol.offset == D["offset"]
    assert sum(len(e[2]) for e in events) == D["streamed"] and len(final[0]) == D["final"]
    assert sum(1 for e in events if len(e[2])) >= 2
    big = O.Volume(D["big"], D["origin0"], D["voxel"])
    big.integrate(d["depth"], d["images"], d["c2w"], DRIVE_K, is_disp=False, near=D["near"], max_depth=D["max_depth"])
    want_xyz, want_rgb, _ = big.extract(D["min_weight"])
    got = sorted(sum((rows(e[2], e[3]) for e in events), []) + rows(*final))
    assert len(got) == D["streamed"] + D["final"] == len(want_xyz) and got == rows(want_xyz, want_rgb)
    return events, final, vol


def check_drive(backend, frames_per_launch):
    """the kernels reproduce the rolled run bit for bit, in emission order"""
    D = DRIVE
    want_events, want_final, want_vol = drive_reference()
    vol = backend.rolling(D["window"], D["origin0"], D["voxel"], frames_per_launch)
    events, final, vol = run_drive(vol, backend.shift_for, backend.dev, backend.host, frames_per_launch)
    assert [(e[0], e[1]) for e in events] == [(e[0], e[1]) for e in want_events]
    assert len(events) == D["shifts"] and tuple(vol.offset) == D["offset"]
    for got, want in zip(events, want_events):
        assert same_bits(got[2], want[2]) and same_bits(got[3], want[3]), ("shift", got[0], got[1])
    assert same_bits(final[0], want_final[0]) and same_bits(final[1], want_final[1])
    assert sum(len(e[2]) for e in events) == D["streamed"] and len(final[0]) == D["final"]
    assert same_bits(backend.host(vol.planes), want_vol.planes)
    assert tuple(f32(o) for o in vol.origin) == tuple(want_vol.origin)
    return events


# ---- rejected arguments ----

def rejections(dims=DIMS):
    """(nx, ny, nz, src offset, dst offset) into one buffer of 2 x 5 nvox + 8 floats; None: a NULL pointer"""
    nx, ny, nz = dims
    size = 5 * nx * ny * nz
    return [(nx, ny, nz, 0, 0), (nx, ny, nz, 0, size // 2), (nx, ny, nz, size // 2, 0), (nx, ny, nz, 0, size - 1),
            (nx, ny, nz, 4, 0), (0, ny, nz, 0, size), (nx, -1, nz, 0, size), (nx, ny, 0, 0, size),
            (1024, 1024, 513, 0, size), (65536, 65536, 1, 0, size), (nx, ny, nz, None, size), (nx, ny, nz, 0, None)]
