"""scsfm_hip.rolling (libscsfm_roll.so) on the device against tests/rolling_oracle.py, bit for bit: the cases of
tests/_roll_cases.py, which tests/test_rolling_hostsim.py runs on the host simulator -- the shift, the extraction of the
crossings that leave (an empty keep box also against libscsfm_fuse.so itself), the partition, rejected arguments, the
moving window against one big volume; then what only the device shows -- guard bands round the outputs, RollingVolume and
its refusals, the other wrappers on a volume that has moved, and reconstruct.py --follow end to end."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import _roll_cases as C
import rolling_oracle as RO

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 64
f32 = np.float32


def _dev(a, dtype=None):
    return torch.from_numpy(np.array(a, dtype)).to(DEV)   # (np.array copies: the cases are read-only)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _call(name, *args):
    from scsfm_hip import _lib
    _lib.get_roll().call(name, *args)


class Backend:
    """the library's entry points on device tensors; every output has GUARD elements of NaN (0xAB for bytes) in front of
    it and behind it, which must stay as they were, and the inputs must keep their bits"""

    @staticmethod
    def shift(planes, s, lead=0):
        """``lead``: dst starts that many floats past a 16-byte boundary"""
        from scsfm_hip.fusion import _ptr, _stream
        _, nz, ny, nx = planes.shape
        src = _dev(planes)
        before = _bits(src).clone()
        buf = torch.full((planes.size + 2 * GUARD + lead,), float("nan"), dtype=torch.float32, device=DEV)
        assert buf.data_ptr() % 16 == 0
        dst = buf[GUARD + lead:GUARD + lead + planes.size]
        _call("scsfm_roll_shift", nx, ny, nz, *(int(v) for v in s), _ptr(src), _ptr(dst), _stream(src.device))
        assert bool(torch.isnan(buf[:GUARD + lead]).all()) and bool(torch.isnan(buf[GUARD + lead + planes.size:]).all()), "shift: guard"
        assert torch.equal(_bits(src), before), "the shift changed its source"
        return dst.reshape(planes.shape).cpu().numpy()

    @staticmethod
    def leaving(planes, dims, origin, voxel, box, min_weight=1.0, capacity=None):
        from scsfm_hip import _lib
        from scsfm_hip.fusion import _ptr, _stream
        vol = _dev(planes, np.float32)
        before = _bits(vol).clone()
        lib = _lib.get_roll()
        n = lib.size("scsfm_roll_ws_bytes", *dims)
        assert n > 0 and n % 4 == 0 and n == _lib.get_fuse().size("scsfm_fuse_extract_ws_bytes", *dims)
        ints = n // 4
        wbuf = torch.full((ints + 2 * GUARD,), -7, dtype=torch.int32, device=DEV)
        ws = wbuf[GUARD:GUARD + ints]
        stream = _stream(vol.device)
        lib.call("scsfm_roll_count", *dims, *box, _ptr(vol), float(min_weight), _ptr(ws), n, stream)
        total = int(ws[0].item())
        cap = total if capacity is None else int(capacity)
        xbuf = torch.full((3 * cap + 2 * GUARD,), float("nan"), dtype=torch.float32, device=DEV)
        cbuf = torch.full((3 * cap + 2 * GUARD,), 0xAB, dtype=torch.uint8, device=DEV)
        xyz, rgb = xbuf[GUARD:GUARD + 3 * cap], cbuf[GUARD:GUARD + 3 * cap]
        lib.call("scsfm_roll_extract", *dims, *(float(f32(o)) for o in origin), float(f32(voxel)), *box, _ptr(vol),
                 float(min_weight), _ptr(ws), n, cap, _ptr(xyz) if cap else None, _ptr(rgb) if cap else None, stream)
        assert bool((wbuf[:GUARD] == -7).all()) and bool((wbuf[GUARD + ints:] == -7).all()) and bool((ws[1:4] == -7).all())
        assert bool(torch.isnan(xbuf[:GUARD]).all()) and bool(torch.isnan(xbuf[GUARD + 3 * cap:]).all()), "xyz: guard"
        assert bool((cbuf[:GUARD] == 0xAB).all()) and bool((cbuf[GUARD + 3 * cap:] == 0xAB).all()), "rgb: guard"
        assert torch.equal(_bits(vol), before), "the extraction changed the volume"
        return total, ws.cpu().numpy(), xyz.reshape(cap, 3).cpu().numpy(), rgb.reshape(cap, 3).cpu().numpy()

    @staticmethod
    def rolling(dims, origin0, voxel, frames_per_launch):
        from scsfm_hip import rolling
        return rolling.RollingVolume(dims, origin0, voxel, device=DEV, frames_per_launch=frames_per_launch)

    @staticmethod
    def shift_for(*args):
        from scsfm_hip import rolling
        return rolling.shift_for(*args)

    dev = staticmethod(lambda a: _dev(a))
    host = staticmethod(lambda t: t.cpu().numpy())


@pytest.mark.parametrize("case", C.SHIFT_CASES, ids=C.shift_id)
def test_shift_equals_the_oracle_bit_for_bit(case):
    C.check_shift(case, Backend)


@pytest.mark.parametrize("case", C.LEAVING_CASES, ids=lambda c: "{}-{:g}-{}".format(*c))
def test_leaving_extraction_equals_the_oracle_bit_for_bit(case):
    total = C.check_leaving(case, Backend)
    name, min_weight, box_name = case
    if box_name.startswith("empty"):
        # and libscsfm_fuse.so itself: the workspace and the points
        from scsfm_hip import fusion
        ref = C.F.reference(name)[0]
        vol = fusion.Volume(ref.dims, ref.origin, ref.voxel, device=DEV)
        vol.planes.copy_(_dev(ref.planes))
        n, ws = vol.count(min_weight)
        mine = Backend.leaving(ref.planes, ref.dims, ref.origin, ref.voxel, C.boxes()[box_name], min_weight)
        ws = ws.cpu().numpy()
        assert n == total and ws[0] == mine[1][0] and np.array_equal(ws[4:], mine[1][4:])
        xyz, rgb = vol.extract(min_weight)
        assert C.same_bits(xyz.cpu().numpy(), mine[2]) and C.same_bits(rgb.cpu().numpy(), mine[3])


@pytest.mark.parametrize("s", C.shifts(), ids=lambda s: "{},{},{}".format(*s))
def test_leaving_and_kept_crossings_partition_the_extraction(s):
    C.check_partition(s, Backend)


def test_rejected_arguments_return_minus_one_and_touch_nothing():
    from scsfm_hip import _lib
    lib = _lib.get_roll()
    size = 5 * int(np.prod(C.DIMS))
    buf = torch.arange(2 * size + 8, dtype=torch.float32, device=DEV)
    before = buf.clone()
    base = buf.data_ptr()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for nx, ny, nz, a, b in C.rejections():
        src = None if a is None else ctypes.c_void_p(base + 4 * a)
        dst = None if b is None else ctypes.c_void_p(base + 4 * b)
        assert lib._fn["scsfm_roll_shift"](nx, ny, nz, 1, 0, -1, src, dst, stream) == -1, (nx, ny, nz, a, b)
    assert lib._fn["scsfm_roll_shift"](*C.DIMS, 0, 0, 0, ctypes.c_void_p(base + 2), ctypes.c_void_p(base + 4 * size + 16),
                                       stream) == -1
    assert torch.equal(buf, before)
    # two buffers that touch without overlapping are accepted
    assert lib._fn["scsfm_roll_shift"](*C.DIMS, 0, 0, 0, ctypes.c_void_p(base), ctypes.c_void_p(base + 4 * size), stream) == 0
    assert torch.equal(buf[size:2 * size], before[:size]) and torch.equal(buf[:size], before[:size])
    assert torch.equal(buf[2 * size:], before[2 * size:])


@pytest.mark.parametrize("frames_per_launch", (1, 8))
def test_the_moving_window_equals_one_big_volume(frames_per_launch):
    """C.drive_reference() holds the issue's conditions on the oracle (10 shifts to (16, 0, 64), 519 points streamed out
    and 708 at the end, the 1227 rows those of one 56 x 16 x 112 volume); RollingVolume, placed by
    scsfm_hip.rolling.shift_for, reproduces the rolled run bit for bit, in emission order."""
    events = C.check_drive(Backend, frames_per_launch)
    assert [len(e[2]) for e in events] == [0, 0, 0, 0, 0, 90, 144, 142, 0, 143]


def test_a_shift_past_the_whole_volume_and_a_larger_one():
    """512 x 64 x 96 voxels (63 MB of planes: 12 288 workgroups of the shift) against torch's slice copy, by bits"""
    from scsfm_hip import rolling
    vol = rolling.RollingVolume((512, 64, 96), (0.0, 0.0, 0.0), 0.25, device=DEV)
    gen = torch.Generator(device=DEV).manual_seed(7)
    vol.planes.copy_(torch.randint(-2 ** 31, 2 ** 31 - 1, vol.planes.shape, dtype=torch.int64, device=DEV,
                                   generator=gen).to(torch.int32).view(torch.float32))
    before = vol.planes.clone()
    vol.move((5, -3, 8))
    want = torch.zeros_like(before)
    want[:, :88, 3:, :507] = before[:, 8:, :61, 5:]
    assert torch.equal(_bits(vol.planes), _bits(want)) and vol.offset == (5, -3, 8) and vol.origin == (1.25, -0.75, 2.0)
    vol.move((0, 0, -96))
    assert not _bits(vol.planes).any() and vol.offset == (5, -3, -88)


def test_rolling_volume_and_the_other_wrappers_on_a_volume_that_has_moved():
    from scsfm_hip import confidence, fusion, raycast, rolling
    d, D = C.drive(), C.DRIVE
    with pytest.raises(TypeError, match="HIP device"):
        rolling.RollingVolume(D["window"], D["origin0"], D["voxel"], device="cpu")
    with pytest.raises(ValueError, match="2\\^29"):
        rolling.RollingVolume((1024, 1024, 513), D["origin0"], D["voxel"], device=DEV)
    vol = rolling.RollingVolume(D["window"], D["origin0"], D["voxel"], device=DEV)
    assert vol.nbytes == 40 * 40 * 16 * 48 and vol.offset == (0, 0, 0) and vol.origin == vol.origin0 == D["origin0"]
    K = _dev(C.DRIVE_K)
    depth, images, c2w = _dev(d["depth"][:24]), _dev(d["images"][:24]), _dev(d["c2w"][:24])
    with pytest.raises(TypeError, match="HIP device"):
        vol.integrate(depth.cpu(), images, c2w, K, is_disp=False)
    with pytest.raises(TypeError, match="float32"):
        vol.integrate(depth.double(), images, c2w, K, is_disp=False)
    with pytest.raises(ValueError, match="contiguous"):
        vol.integrate(depth.transpose(1, 2), None, c2w, K, is_disp=False)
    with pytest.raises(ValueError, match="three"):
        vol.shift((8, 0))
    assert not vol.planes.any()                       # (a refused call touches nothing)
    kw = dict(is_disp=False, near=D["near"], max_depth=D["max_depth"])
    vol.integrate(depth, images, c2w, K, **kw)
    held = vol.planes
    xyz, rgb = vol.shift((8, 0, 16), 1.0)
    assert vol.offset == (8, 0, 16) and vol.origin == (-1.5, -1.0, -1.0) and vol.planes.data_ptr() != held.data_ptr()
    assert xyz.dtype == torch.float32 and rgb.dtype == torch.uint8 and xyz.shape == rgb.shape and xyz.is_cuda
    # the same calls on a fresh fusion.Volume given the planes and the current origin
    w = torch.rand((4, 12, 20), device=DEV, generator=torch.Generator(device=DEV).manual_seed(1))
    # (early frames: the floor they see, 1.3 to 1.5 ahead of them, lay inside the first window and was kept by the move)
    more = (_dev(d["depth"][4:8]), _dev(d["images"][4:8]), _dev(d["c2w"][4:8]), K)
    plain = fusion.Volume(vol.dims, vol.origin, vol.voxel, vol.trunc, device=DEV)
    plain.planes.copy_(vol.planes)
    got = vol.track(more[0], more[2], K, is_disp=False, near=D["near"], max_depth=D["max_depth"], iterations=3)
    want = plain.track(more[0], more[2], K, is_disp=False, near=D["near"], max_depth=D["max_depth"], iterations=3)
    assert torch.equal(got.c2w, want.c2w) and torch.equal(_bits(got.report), _bits(want.report))
    assert torch.equal(_bits(got.model_depth), _bits(want.model_depth)) and bool((got.model_depth > 0).any())
    mask = raycast.brick_mask(vol, 1.0)
    assert torch.equal(mask, raycast.brick_mask(plain, 1.0))
    far = D["max_depth"] + vol.trunc
    a = vol.raycast(more[2], K, C.DRIVE_HW, D["near"], far, mask=mask)
    b = plain.raycast(more[2], K, C.DRIVE_HW, D["near"], far)
    assert torch.equal(_bits(a.depth), _bits(b.depth)) and torch.equal(a.rgb, b.rgb) and bool((a.depth > 0).any())
    vol.integrate(*more, weight=w, **kw)
    confidence.integrate(plain, *more, w, **kw)
    assert torch.equal(_bits(vol.planes), _bits(plain.planes))
    vol.integrate(*more, **kw)
    plain.integrate(*more, **kw)
    assert torch.equal(_bits(vol.planes), _bits(plain.planes))
    for x, y in zip(vol.extract(1.0), plain.extract(1.0)):
        assert torch.equal(x, y) and len(x) > 100


def _files(folder):
    return sorted(os.listdir(str(folder)))


def _read_ply(path):
    blob = open(str(path), "rb").read()
    head, body = blob.split(b"end_header\n", 1)
    n = int(re.search(rb"element vertex (\d+)", head).group(1))
    rec = np.frombuffer(body, dtype=[("xyz", "<f4", 3), ("rgb", "u1", 3)])
    assert len(rec) == n
    return rec["xyz"], rec["rgb"]


def test_reconstruct_follow_on_twelve_generated_frames(tmp_path, capsys):
    """reconstruct.py --follow on twelve generated 64 x 96 frames with randomly initialised nets saved by the test (the
    setting of tests/test_gpu_confidence.py's end-to-end test: this is about plumbing and determinism).  A random pose net
    barely moves, and the window would never shift, so the saved PoseResNet's last convolution gets a bias that makes
    every pair a forward motion of 0.25, five voxels of 0.05.  A plain run writes exactly poses.txt and
    reconstruction.ply and prints its three lines.  With --follow (a window of 24 voxels a side, so that points leave it
    within twelve frames) poses.txt keeps its bytes; on_shift sees at least two moves; reconstruction.ply is the hooks'
    points in order and then the returned volume's extraction; the returned volume equals a fresh RollingVolume driven by
    the hooks' batches and shifts, whose shifts give the hooks' points; a second run writes the same files.  With
    --consistency-weight --refine-poses --refine-group 2 added the run completes and is reproduced by its hooks in the
    same way, every batch with its rows of the weights."""
    from PIL import Image

    import models
    import reconstruct
    from scsfm_hip import rolling
    torch.manual_seed(4)
    rng = np.random.default_rng(4)
    frames = tmp_path / "frames"
    frames.mkdir()
    yy, xx = np.mgrid[:64, :96]
    for k in range(12):
        base = 128 + 60 * np.sin((xx + 7 * k) / 9.0)[..., None] * np.cos(yy / 11.0)[..., None]
        Image.fromarray(np.clip(base + rng.normal(0, 12, (64, 96, 3)), 0, 255).astype(np.uint8)).save(
            str(frames / f"{k:06d}.png"))
    torch.save({"state_dict": models.DispResNet(18, False).state_dict()}, str(tmp_path / "disp.pth.tar"))
    pose = models.PoseResNet(18, False)
    with torch.no_grad():
        pose.decoder.net[3].bias[2] = 25.0          # the pose vector is 0.01 times the mean: tz = 0.25 more
    torch.save({"state_dict": pose.state_dict()}, str(tmp_path / "pose.pth.tar"))
    np.savetxt(str(tmp_path / "cam.txt"), np.array([[58.0, 0, 47.5], [0, 58.0, 31.5], [0, 0, 1]]))
    argv = ["--pretrained-dispnet", str(tmp_path / "disp.pth.tar"), "--pretrained-posenet", str(tmp_path / "pose.pth.tar"),
            "--dataset-dir", str(frames), "--intrinsics", str(tmp_path / "cam.txt"), "--img-height", "64", "--img-width",
            "96", "--batch-size", "4", "--max-depth", "2.0", "--voxel-size", "0.05", "--min-weight", "1",
            "--frames-per-launch", "2", "--refine-iterations", "3"]
    follow = ["--follow", "--follow-dims", "24", "24", "24"]
    runs = {}
    old = torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = True, False
    try:
        reconstruct.main(argv + ["--output-dir", str(tmp_path / "plain")])
        plain_out = capsys.readouterr().out
        for name, extra in (("a", follow), ("b", follow),
                            ("all", follow + ["--consistency-weight", "--refine-poses", "--refine-group", "2"])):
            seen = {"events": [], "weights": []}
            vol = reconstruct.main(
                argv + extra + ["--output-dir", str(tmp_path / name)],
                on_batch=lambda *t, s=seen: s["events"].append(("batch", [x.clone() for x in t])),
                on_shift=lambda sh, off, xyz, rgb, s=seen: s["events"].append(("shift", sh, off, xyz.clone(), rgb.clone())),
                on_weights=lambda w, d, s=seen: s["weights"].append(w.clone()))
            runs[name] = (vol, seen, capsys.readouterr().out)
        for bad, words in ((["--follow", "--mesh"], "--mesh"), (["--follow-step", "4"], "needs --follow")):
            with pytest.raises(SystemExit, match=words):
                reconstruct.main(argv + bad + ["--output-dir", str(tmp_path / "bad")])
    finally:
        torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = old
    plain = tmp_path / "plain"
    assert _files(plain) == ["poses.txt", "reconstruction.ply"] and not (tmp_path / "bad").exists()
    lines = plain_out.splitlines()
    assert len(lines) == 3 and lines[0] == "12 files to reconstruct from", lines
    assert re.fullmatch(r"volume: \d+ x \d+ x \d+ voxels of 0\.05, \d+\.\d MB, corner \(\S+, \S+, \S+\)", lines[1]), lines[1]
    assert re.fullmatch(r"\d+ surface points from 12 frames -> " + re.escape(str(plain / "reconstruction.ply")), lines[2])
    chain = np.loadtxt(str(plain / "poses.txt")).reshape(-1, 3, 4)
    steps = np.linalg.norm(np.diff(chain[:, :, 3], axis=0), axis=1)
    assert (steps > 0.2).all() and (steps < 0.3).all(), steps         # a few voxels of 0.05 a pair
    for name, (vol, seen, printed) in runs.items():
        out = tmp_path / name
        assert _files(out) == ["poses.txt"] + (["poses_refined.txt"] if name == "all" else []) + ["reconstruction.ply"]
        assert (out / "poses.txt").read_bytes() == (plain / "poses.txt").read_bytes()
        assert isinstance(vol, rolling.RollingVolume) and vol.dims == (24, 24, 24)
        shifts = [e for e in seen["events"] if e[0] == "shift"]
        batches = [e for e in seen["events"] if e[0] == "batch"]
        assert len(shifts) >= 2 and all(any(e[1]) and all(v % 8 == 0 for v in e[1]) for e in shifts), name
        assert [len(b[1][0]) for b in batches] == ([1, 2, 2, 2, 2, 2, 1] if name == "all" else [4, 4, 4])
        # the file: the hooks' points in order, then the returned volume's extraction
        last = vol.extract(1.0)
        xyz = np.concatenate([e[3].cpu().numpy() for e in shifts] + [last[0].cpu().numpy()])
        rgb = np.concatenate([e[4].cpu().numpy() for e in shifts] + [last[1].cpu().numpy()])
        file_xyz, file_rgb = _read_ply(out / "reconstruction.ply")
        assert C.same_bits(file_xyz, xyz) and C.same_bits(file_rgb, rgb), name
        streamed = sum(len(e[3]) for e in shifts)
        print(f"{name}: {len(shifts)} shifts {[e[1] for e in shifts]}, {streamed} points streamed out, {len(last[0])} at the end")
        assert streamed > 0 and len(last[0]) > 0, name
        assert len(set(C.rows(xyz, rgb))) == len(xyz), name           # (no point twice)
        # a fresh volume driven by the hooks
        fresh = rolling.RollingVolume(vol.dims, vol.origin0, vol.voxel, vol.trunc, device=DEV, frames_per_launch=2)
        weights = seen["weights"][0] if name == "all" else None
        assert (weights is None) == (not seen["weights"])
        at = 0
        for e in seen["events"]:
            if e[0] == "shift":
                got = fresh.shift(e[1], 1.0)
                assert torch.equal(_bits(got[0]), _bits(e[3])) and torch.equal(got[1], e[4]) and fresh.offset == tuple(e[2])
            else:
                n = len(e[1][0])
                fresh.integrate(*e[1], is_disp=True, max_depth=2.0, weight=None if weights is None else weights[at:at + n])
                at += n
        assert at == 12 and fresh.offset == vol.offset and fresh.origin == vol.origin
        assert torch.equal(_bits(fresh.planes), _bits(vol.planes)), name
        assert vol.origin == rolling.origin_at(vol.origin0, vol.offset, vol.voxel)
        # the printed lines: the window instead of the box, the shifts beside the points
        assert "volume:" not in printed
        assert re.search(r"^window: 24 x 24 x 24 voxels of 0\.05, 0\.6 MB, first corner \(\S+, \S+, \S+\)$", printed, re.M), printed
        assert re.search(r"^{} surface points from 12 frames -> ".format(len(xyz)), printed, re.M), printed
        assert "the window moved {} times to offset ({}, {}, {}); {} of the points were streamed out on the way".format(
            len(shifts), *vol.offset, streamed) in printed
    # without --refine-poses the window is placed from the chain's poses of frames 2, 6 and 10: the policy, on the host
    vol, seen, _ = runs["a"]
    offset, moves = (0, 0, 0), []
    for k in (2, 6, 10):
        s = RO.shift_for(chain[k][:, 3], vol.origin0, offset, vol.dims, vol.voxel, 8)
        if any(s):
            offset = tuple(a + b for a, b in zip(offset, s))
            moves.append((s, offset))
    assert moves == [(e[1], tuple(e[2])) for e in seen["events"] if e[0] == "shift"]
    assert vol.origin0 == tuple(float(f32(v)) for v in RO.initial_origin(chain[2][:, 3], vol.dims, 0.05))
    for path in ("poses.txt", "reconstruction.ply"):
        assert (tmp_path / "a" / path).read_bytes() == (tmp_path / "b" / path).read_bytes(), path
