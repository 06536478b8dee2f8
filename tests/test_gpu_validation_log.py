"""libscsfm_vlog.so on the device, through scsfm_hip.validation_log: every entry point and tensor2array against what the
reference recorded in tests/golden/validation_log.npz (equal bits, NaN for NaN, no pixel left out: the arithmetic is all
correctly rounded float32, so equality is the specification), non-contiguous and [N, 1, H, W] inputs, the byte pictures
against the float pictures pushed through the byte rule, and one validate_with_gt and one validate_without_gt run with
--log-output's writers: the files they leave, what each PNG decodes to, and that the returned errors do not change."""
import os
import types

import numpy as np
import pytest
import torch
from PIL import Image

import _validation_log_golden as G
import validation_log_oracle as O

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")


def same(a, b):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    b = np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


def as_pixels(floats):
    return np.ascontiguousarray(O.to_bytes(floats).transpose(0, 2, 3, 1))


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)


@pytest.mark.parametrize("key", ["a", "b", "c"])
def test_map_pictures_and_tensor2array_equal_the_golden(key):
    from scsfm_hip import validation_log as VL
    g = G.load()
    maps = dev(g[f"maps_{key}"])
    for cmap, max_value in G.CALLS:
        want = g[f"{key}/{cmap}"]
        floats, rgba = VL.map_pictures(maps, cmap, max_value)
        assert floats.is_cuda and rgba.is_cuda and floats.is_contiguous() and rgba.is_contiguous()
        assert same(floats, want), (cmap, np.argwhere(floats.cpu().numpy() != want)[:4].tolist())
        assert same(rgba, as_pixels(want)), cmap
        assert same(VL.map_pictures(maps, cmap, max_value, bytes_=False)[0], want)
        only = VL.map_pictures(maps, cmap, max_value, floats=False)
        assert only[0] is None and torch.equal(only[1], rgba)
        for n in range(len(maps)):  # the reference's dispatch: [H, W] and [1, H, W]
            for t in (maps[n], maps[n][None]):
                got = VL.tensor2array(t, max_value, cmap) if max_value is not None else VL.tensor2array(t, colormap=cmap)
                assert got.is_cuda and same(got, want[n]), (cmap, n)
    with np.errstate(invalid="ignore"):
        want_max = g[f"maps_{key}"].reshape(len(maps), -1).max(axis=1)
    got_max = VL.image_max(maps).cpu().numpy()
    assert bool(np.all((got_max == want_max) | (np.isnan(got_max) & np.isnan(want_max))))


def test_non_contiguous_four_dimensional_and_offset_inputs():
    from scsfm_hip import validation_log as VL
    g = G.load()
    a = g["maps_a"]
    wide = np.full((6, 9, 20), 99.0, np.float32)
    wide[:, :, 3:16] = a
    view = dev(wide)[:, :, 3:16]
    assert not view.is_contiguous()
    four = dev(a)[:, None]  # [N, 1, H, W]
    flat = torch.cat([torch.zeros(1, device=DEV), dev(a).reshape(-1)])
    off = flat[1:].reshape(6, 9, 13)  # contiguous, 4 bytes past the allocation's boundary
    assert off.is_contiguous() and off.data_ptr() % 16 == 4
    for maps in (view, four, off):
        for cmap, max_value in G.CALLS:
            floats, rgba = VL.map_pictures(maps, cmap, max_value)
            assert same(floats, g[f"a/{cmap}"]) and same(rgba, as_pixels(g[f"a/{cmap}"])), cmap
    # image 1 alone, as train.py takes image 0 of a batch: a [1, H, W] slice of a [N, 1, H, W] network output
    assert same(VL.map_pictures(four[1], "magma")[0], g["a/magma"][1:2])
    batch = g["batch"]
    padded = np.zeros((2, 3, 5, 16), np.float32)
    padded[..., 2:13] = batch
    view = dev(padded)[..., 2:13]
    assert not view.is_contiguous()
    floats, rgb = VL.input_pictures(view)
    assert same(floats, g["batch/floats"]) and same(rgb, as_pixels(g["batch/floats"]))
    gt = np.zeros((2, 9, 15), np.float32)
    gt[..., 1:14] = g["gt"]
    assert same(VL.target_disparity(dev(gt)[..., 1:14]), g["gt/disparity"])


def test_input_picture_on_every_byte_value():
    from scsfm_hip import validation_log as VL
    g = G.load()
    batch, want = dev(g["batch"]), g["batch/floats"]
    floats, rgb = VL.input_pictures(batch)
    assert floats.is_cuda and rgb.is_cuda and rgb.shape == (2, 5, 11, 3) and rgb.dtype == torch.uint8
    assert same(floats, want) and same(rgb, as_pixels(want))
    assert VL.input_pictures(batch, floats=False)[0] is None and torch.equal(VL.input_pictures(batch, floats=False)[1], rgb)
    assert same(VL.input_pictures(batch, bytes_=False)[0], want)
    for n in range(2):
        assert same(VL.tensor2array(batch[n]), want[n])
    assert same(batch, g["batch"])  # (the input is not written)


def test_target_disparity_and_its_pictures():
    from scsfm_hip import validation_log as VL
    g = G.load()
    gt = dev(g["gt"])
    disp = VL.target_disparity(gt)
    assert disp.is_cuda and same(disp, g["gt/disparity"])
    assert same(gt, g["gt"])  # without the reference's in-place write
    assert same(VL.map_pictures(gt, "rainbow", 10)[0], g["gt/depth_picture"])
    floats, rgba = VL.map_pictures(disp, "magma")
    assert same(floats, g["gt/disparity_picture"]) and same(rgba, as_pixels(g["gt/disparity_picture"]))
    assert same(VL.tensor2array(gt[0], max_value=10), g["gt/depth_picture"][0])


def test_non_default_stream_and_repeated_calls():
    from scsfm_hip import validation_log as VL
    g = G.load()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        maps = dev(g["maps_a"])
        first = VL.map_pictures(maps, "magma")
        second = VL.map_pictures(maps, "magma")
    stream.synchronize()
    assert same(first[0], g["a/magma"]) and torch.equal(first[1], second[1])
    assert torch.equal(first[0].view(torch.int32), second[0].view(torch.int32))


# ---- the two validation loops with --log-output's writers ----

H, W = 16, 24


class RecordingDisp(torch.nn.Module):
    """Stands in for DispResNet in eval mode: a disparity in (0.01, 10.01) that depends on the input and on ``gain``
    (which the test changes from epoch to epoch), and a record of every output."""

    def __init__(self):
        super().__init__()
        self.gain, self.outs = 1.0, []

    def forward(self, x):
        self.outs.append(10 * torch.sigmoid(self.gain * x.mean(dim=1, keepdim=True)) + 0.01)
        return self.outs[-1]


class StillPose(torch.nn.Module):
    def forward(self, a, b):
        return torch.full((a.shape[0], 6), 0.01, device=a.device)


def _logger():
    return types.SimpleNamespace(valid_bar=types.SimpleNamespace(update=lambda i: None),
                                 valid_writer=types.SimpleNamespace(write=lambda s: None))


def _decode(path):
    with Image.open(path) as im:
        return im.mode, np.asarray(im).copy()


def _files(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)


def _expected_files(epoch0_only):
    both = ("val_Dispnet_Output_Normalized", "val_Depth_Output")
    return sorted([os.path.join(str(i), tag, "0000.png") for i in range(3) for tag in epoch0_only + both] +
                  [os.path.join(str(i), tag, "0001.png") for i in range(3) for tag in both])


def _check_common(root, i, img, disp_shown, depth_shown):
    """Writer i's three pictures of both loops: the input of epoch 0, and per epoch the two maps."""
    g = G.load()
    mode, got = _decode(os.path.join(root, str(i), "val_Input", "0000.png"))
    assert mode == "RGB" and np.array_equal(got, O.input_bytes(img[:1].numpy())[0])
    for epoch in (0, 1):
        mode, got = _decode(os.path.join(root, str(i), "val_Dispnet_Output_Normalized", f"{epoch:04d}.png"))
        assert mode == "RGBA" and np.array_equal(got, O.map_bytes(disp_shown[epoch][None], g["magma"])[0]), (i, epoch)
        mode, got = _decode(os.path.join(root, str(i), "val_Depth_Output", f"{epoch:04d}.png"))
        assert mode == "RGBA" and np.array_equal(got, O.map_bytes(depth_shown[epoch][None], g["rainbow"], 10)[0]), (i, epoch)
    assert not np.array_equal(disp_shown[0], disp_shown[1])  # (the two epochs show different maps)


def test_validate_with_gt_writes_the_reference_pictures(tmp_path):
    import train as T
    from scsfm_hip import validation_log as VL
    g = G.load()
    rng = np.random.default_rng(31)
    torch.manual_seed(31)
    loader = []
    for _ in range(4):
        gt = rng.uniform(0.05, 90.0, (2, 11, 17)).astype(np.float32)
        gt[rng.random(gt.shape) < 0.3] = 0
        loader.append((torch.randn(2, 3, H, W), torch.tensor(gt)))
    args = types.SimpleNamespace(dataset="kitti", print_freq=1)
    T.device = DEV
    root = str(tmp_path / "valid")

    def run(writers):
        net, out = RecordingDisp(), []
        for epoch in (0, 1):
            net.gain = 1.0 + epoch
            out.append(T.validate_with_gt(args, loader, net, epoch, _logger(), writers))
        return net, out

    net, logged = run([VL.PictureLog(os.path.join(root, str(i))) for i in range(3)])
    _, plain = run([])
    assert logged == plain and len(logged[0][0]) == 6 and np.isfinite(logged[0][0]).all()  # the same errors, bit for bit
    assert len(net.outs) == 8 and tuple(net.outs[0].shape) == (2, 1, H, W)
    assert _files(root) == _expected_files(("val_Input", "val_target_Depth", "val_target_Disparity_Normalized"))
    one = np.float32(1)
    for i in range(3):
        img, gt = loader[i]
        disp = [net.outs[4 * epoch + i][0, 0].cpu().numpy() for epoch in (0, 1)]
        _check_common(root, i, img, disp, [one / d for d in disp])
        mode, got = _decode(os.path.join(root, str(i), "val_target_Depth", "0000.png"))
        assert mode == "RGBA" and got.shape == (11, 17, 4)
        assert np.array_equal(got, O.map_bytes(gt[:1].numpy(), g["rainbow"], 10)[0])
        mode, got = _decode(os.path.join(root, str(i), "val_target_Disparity_Normalized", "0000.png"))
        assert mode == "RGBA" and np.array_equal(got, O.map_bytes(O.target_disparity(gt[:1].numpy()), g["magma"])[0])
        assert torch.equal(gt, loader[i][1]) and (gt == 0).any()  # the ground truth keeps its zeros


def test_validate_without_gt_writes_the_reference_pictures(tmp_path):
    import train as T
    from scsfm_hip import validation_log as VL
    torch.manual_seed(32)
    K = torch.tensor([[20.0, 0, 12], [0, 20.0, 8], [0, 0, 1]]).expand(2, 3, 3).contiguous()
    loader = [(torch.randn(2, 3, H, W), [torch.randn(2, 3, H, W), torch.randn(2, 3, H, W)], K, torch.inverse(K))
              for _ in range(4)]
    args = types.SimpleNamespace(num_scales=1, with_ssim=1, with_mask=1, padding_mode="zeros", print_freq=1)
    T.device = DEV
    root = str(tmp_path / "valid")

    def run(writers):
        net, out = RecordingDisp(), []
        for epoch in (0, 1):
            net.gain = 1.0 + epoch
            out.append(T.validate_without_gt(args, loader, net, StillPose(), epoch, _logger(), writers))
        return net, out

    net, logged = run([VL.PictureLog(os.path.join(root, str(i))) for i in range(3)])
    _, plain = run([])
    assert logged == plain and logged[0][1] == ['Total loss', 'Photo loss', 'Smooth loss', 'Consistency loss']
    assert np.isfinite(logged[0][0]).all()
    assert len(net.outs) == 2 * 4 * 3  # per batch the target first, then the two references
    assert _files(root) == _expected_files(("val_Input",))
    one = np.float32(1)
    for i in range(3):
        # the loop holds depth = 1 / disp and shows 1 / depth as the disparity (train.py:322, :333 of the reference)
        depth = [one / net.outs[12 * epoch + 3 * i][0, 0].cpu().numpy() for epoch in (0, 1)]
        _check_common(root, i, loader[i][0], [one / d for d in depth], depth)
