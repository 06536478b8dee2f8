"""libscsfm_roll.so's kernels on the host simulator (tests/_hostsim_roll.py) against tests/rolling_oracle.py, bit for bit:
the cases of tests/_roll_cases.py, which tests/test_gpu_rolling.py runs on the device -- the shift, the extraction of the
crossings that leave, the partition of a volume's crossings by a keep box, rejected arguments, and a window that moves
along a drive of 80 frames against one big volume on the same lattice."""
import ctypes

import numpy as np
import pytest

import _hostsim_fuse as HF
import _hostsim_roll as HR
import _roll_cases as C
import fusion_oracle as O
import rolling_oracle as RO


class Backend:
    shift = staticmethod(HR.shift)
    leaving = staticmethod(HR.leaving)
    shift_for = staticmethod(RO.shift_for)
    dev = staticmethod(lambda a: a)
    host = staticmethod(lambda a: a)

    @staticmethod
    def rolling(dims, origin0, voxel, frames_per_launch):
        return HR.RollingVolume(dims, origin0, voxel, frames_per_launch=frames_per_launch)


@pytest.mark.parametrize("case", C.SHIFT_CASES, ids=C.shift_id)
def test_shift_equals_the_oracle_bit_for_bit(case):
    want = C.check_shift(case, Backend)
    dims, s = case
    if any(abs(k) >= n for k, n in zip(s, dims)):
        assert not want.view(np.uint32).any()
    if s == (0, 0, 0):
        assert C.same_bits(want, C.patterns(dims))


def test_the_patterns_hold_what_they_should():
    bits = C.patterns(C.DIMS)
    assert np.isnan(bits).sum() >= 3 and np.isinf(bits).sum() == 2
    tiny = np.abs(bits[np.isfinite(bits)])
    assert ((tiny > 0) & (tiny < np.finfo(np.float32).tiny)).sum() >= 2
    # the oracle's shift against a loop over the voxels of a small volume
    src = C.patterns((5, 3, 4)).view(np.uint32)
    for s in ((1, 0, 0), (-2, 1, 0), (0, -1, 3), (5, 0, 0), (0, 0, -4)):
        want = np.zeros_like(src)
        for z in range(4):
            for y in range(3):
                for x in range(5):
                    a = (x + s[0], y + s[1], z + s[2])
                    if 0 <= a[0] < 5 and 0 <= a[1] < 3 and 0 <= a[2] < 4:
                        want[:, z, y, x] = src[:, a[2], a[1], a[0]]
        assert np.array_equal(RO.shift_planes(src.view(np.float32), s).view(np.uint32), want), s


@pytest.mark.parametrize("case", C.LEAVING_CASES, ids=lambda c: "{}-{:g}-{}".format(*c))
def test_leaving_extraction_equals_the_oracle_bit_for_bit(case):
    total = C.check_leaving(case, Backend)
    name, min_weight, box_name = case
    if box_name == "empty":
        # and libscsfm_fuse's own kernels, on the simulator: the workspace and the points
        ref = C.F.reference(name)[0]
        vol = HF.Volume(ref.dims, ref.origin, ref.voxel)
        vol.planes[...] = ref.planes
        n, ws = vol.count(min_weight)
        mine = HR.leaving(ref.planes, ref.dims, ref.origin, ref.voxel, C.boxes()[box_name], min_weight)
        assert n == total and np.array_equal(ws[:1], mine[1][:1]) and np.array_equal(ws[4:], mine[1][4:])
        xyz, rgb = vol.extract(min_weight)
        assert C.same_bits(xyz, mine[2]) and C.same_bits(rgb, mine[3])


def test_the_leaving_cases_are_not_trivial():
    """on the oracle: in every volume with more than 40 points at least four of the keep boxes let some points leave and
    keep others (the scene's surface lies in the middle of the volume: the first eight slices in z hold none)"""
    for name in C.VOLUMES:
        for w in C.MIN_WEIGHTS:
            full = len(C.leaving_reference(name, w, "empty")[0])
            some = [b for b in C.BOX_NAMES if 0 < len(C.leaving_reference(name, w, b)[0]) < full]
            assert len(some) >= 4 or full <= 40, (name, w, some, full)
    assert len(C.leaving_reference("straddle_F5", 2.0, "empty")[0]) > 40


@pytest.mark.parametrize("s", C.shifts(), ids=lambda s: "{},{},{}".format(*s))
def test_leaving_and_kept_crossings_partition_the_extraction(s):
    C.check_partition(s, Backend)


def test_a_kept_chunk_does_not_load_the_volume():
    """a keep box that covers everything: the volume pointer is never read (it points at nothing), the counts are zeros;
    with the box of the shift (0, 0, 8) in a volume of 2048-voxel slices, only the chunks of the first eight slices and of
    the ninth's lower neighbours are read: the rest of the buffer is not even there"""
    lib = HR.lib()
    dims = (64, 32, 40)                              # a slice is two chunks
    n = lib.size("scsfm_roll_ws_bytes", *dims)
    ws = np.full(n // 4, -1, np.int32)
    nowhere = ctypes.c_void_p(4096)
    assert lib._fn["scsfm_roll_count"](*dims, 0, 64, 0, 32, 0, 40, nowhere, 1.0, HR._ptr(ws), n, None) == 0
    assert ws[0] == 0 and not ws[4:].any()
    # slices 0 .. 8 present (the edges from slice 7 end in slice 8), the others missing
    nvox = 64 * 32 * 40
    rng = np.random.default_rng(3)
    part = np.zeros((2, 9, 32, 64), np.float32)
    part[0] = rng.uniform(-1, 1, part[0].shape)
    part[1] = 1.0
    k = HR._Call()
    # (the weight plane starts nvox floats behind the tsdf plane; only the first nine slices of either are ever addressed,
    # so the buffer ends there, in front of a guard band)
    buf = k.out((nvox + 9 * 2048,))
    buf[:9 * 2048] = part[0].reshape(-1)
    buf[nvox:] = 1.0
    ws[...] = -1
    assert lib._fn["scsfm_roll_count"](*dims, *RO.keep_box(dims, (0, 0, 8)), HR._ptr(buf), 1.0, HR._ptr(ws), n, None) == 0
    k.check("scsfm_roll_count")
    full = O.Volume(dims, (0, 0, 0), 1.0)
    full.planes[0, :9], full.planes[1, :9] = part[0], 1.0
    want = RO.leaving(full, RO.keep_box(dims, (0, 0, 8)), 1.0)
    assert ws[0] == len(want[0]) > 1000 and np.array_equal(ws[4:4 + len(want[2])], want[2])


def test_rejected_arguments_return_minus_one_and_touch_nothing():
    lib = HR.lib()
    size = 5 * int(np.prod(C.DIMS))
    k = HR._Call()
    buf = k.arg(np.arange(2 * size + 8, dtype=np.float32))
    before = buf.copy()
    base = buf.ctypes.data
    for nx, ny, nz, a, b in C.rejections():
        src = None if a is None else ctypes.c_void_p(base + 4 * a)
        dst = None if b is None else ctypes.c_void_p(base + 4 * b)
        k.run("scsfm_roll_shift", nx, ny, nz, 1, 0, -1, src, dst, None, status=-1)
        assert C.same_bits(buf, before), (nx, ny, nz, a, b)
    odd = ctypes.c_void_p(base + 2)
    k.run("scsfm_roll_shift", *C.DIMS, 0, 0, 0, odd, ctypes.c_void_p(base + 4 * size + 16), None, status=-1)
    k.run("scsfm_roll_shift", *C.DIMS, 0, 0, 0, ctypes.c_void_p(base), ctypes.c_void_p(base + 4 * size + 2), None, status=-1)
    assert C.same_bits(buf, before)
    # two buffers that touch without overlapping are accepted
    k.run("scsfm_roll_shift", *C.DIMS, 0, 0, 0, ctypes.c_void_p(base), ctypes.c_void_p(base + 4 * size), None)
    assert C.same_bits(buf[size:2 * size], before[:size]) and C.same_bits(buf[:size], before[:size])
    assert C.same_bits(buf[2 * size:], before[2 * size:])
    # the extraction: sizes, pointers, alignment, min_weight, the workspace's size, the capacity
    n = lib.size("scsfm_roll_ws_bytes", *C.DIMS)
    assert lib.size("scsfm_roll_ws_bytes", 0, 1, 1) == 0 and lib.size("scsfm_roll_ws_bytes", 1024, 1024, 513) == 0
    p, odd = ctypes.c_void_p(4096), ctypes.c_void_p(4100)
    box = (0, 0, 0, 0, 0, 0)
    count, extract = lib._fn["scsfm_roll_count"], lib._fn["scsfm_roll_extract"]
    for args in ((0, 18, 29, *box, p, 1.0, p, n), (37, 18, 29, *box, None, 1.0, p, n), (37, 18, 29, *box, p, 1.0, None, n),
                 (37, 18, 29, *box, p, 1.0, odd, n), (37, 18, 29, *box, p, 0.5, p, n), (37, 18, 29, *box, p, float("nan"), p, n),
                 (37, 18, 29, *box, p, 1.0, p, n - 4), (1024, 1024, 513, *box, p, 1.0, p, n)):
        assert count(*args, None) == -1, args
    good = [37, 18, 29, 0.0, 0.0, 0.0, 0.1, *box, p, 1.0, p, n, 5, p, p]
    for at, bad in ((0, 0), (3, float("nan")), (5, float("inf")), (6, 0.0), (6, -1.0), (13, None), (14, 0.5), (15, None),
                    (15, odd), (16, n - 4), (17, -1), (18, None), (19, None)):
        args = list(good)
        args[at] = bad
        assert extract(*args, None) == -1, (at, bad)
    assert lib._fn["scsfm_roll_source_id"](None, 64) == -1


@pytest.mark.parametrize("frames_per_launch", (1, 8))
def test_the_moving_window_equals_one_big_volume(frames_per_launch):
    """C.drive_reference() holds the issue's conditions on the oracle (10 shifts to (16, 0, 64), 519 points streamed out
    and 708 at the end, the 1227 rows those of one 56 x 16 x 112 volume); the kernels reproduce the rolled run bit for
    bit, in emission order.  On the oracle the points leave with four of the ten shifts: 90, 144, 142 and 143."""
    events = C.check_drive(Backend, frames_per_launch)
    assert [len(e[2]) for e in events] == [0, 0, 0, 0, 0, 90, 144, 142, 0, 143]
