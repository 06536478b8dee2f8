"""Shared by the CPU and the GPU tests of scsfm_hip.prepare: the resize cases and PIL's answer to them, the judgement of
a depth map against the reference's, the fixtures' projection matrices, and generated point clouds."""
from __future__ import annotations

import os

import numpy as np
from PIL import Image

import _prepare_data_tree as T
from _util import report
from scsfm_hip.prepare import velo_projection

# (H, W) -> (h, w), C, keep_rows, N: the cases of the issue
RESIZE_CASES = {
    "7taps_edges": (23, 61, 8, 20, 3, None, 1),
    "11taps_keep9": (59, 205, 12, 41, 3, 9, 1),
    "upscale": (9, 13, 20, 31, 3, None, 1),
    "vertical_skipped": (24, 61, 24, 20, 3, None, 1),
    "horizontal_skipped": (31, 16, 8, 16, 3, None, 1),
    "copy": (12, 12, 12, 12, 3, None, 1),
    "grey": (23, 61, 8, 20, 1, None, 1),
    "four_channels": (23, 61, 8, 20, 4, None, 1),
    "three_frames_tail": (23, 61, 8, 20, 3, None, 3),
    "kitti_ratio": (375, 1242, 128, 416, 3, None, 1),
}
# four independent 8-bit channels (Pillow premultiplies RGBA by its alpha before it resamples; CMYK it does not)
MODES = {1: "L", 3: "RGB", 4: "CMYK"}


def resize_inputs(name):
    H, W, h, w, C, keep, N = RESIZE_CASES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    return rng.integers(0, 256, (N, H, W, C), dtype=np.uint8), h, w, keep


def pil_resize(images, h, w, keep=None):
    out = []
    for img in images:
        C = img.shape[2]
        im = Image.fromarray(img[:, :, 0] if C == 1 else img, MODES[C]).resize((w, h), Image.BILINEAR)
        out.append(np.asarray(im).reshape(h, w, C)[:keep or h])
    return np.stack(out)


def judge_depth(got, want, what):
    """The issue's criterion: the same pattern of zeros, every entry within one float32 ulp (bit equality is expected;
    the allowance covers the unspecified summation order of the reference's BLAS product).  Reports and returns the
    number of entries that differ at all."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == np.float32 and want.dtype == np.float32
    assert np.isfinite(got).all()
    assert np.array_equal(got == 0, want == 0), f"{what}: the pattern of zeros differs"
    ulps = np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))
    differ = int((ulps != 0).sum())
    report(f"prepare depth {what}: {differ} of {got.size} entries differ from the reference (max {int(ulps.max())} ulp)")
    print(f"{what}: {differ} entries differ, max {int(ulps.max())} ulp")
    assert ulps.max() <= 1, f"{what}: {int(ulps.max())} ulp"
    return differ


def read_calib(name):
    out = {}
    for line in open(os.path.join(T.TEXT, name)):
        k, v = line.split(":", 1)
        try:
            out[k] = np.array([float(x) for x in v.split()])
        except ValueError:
            pass
    return out


def golden_projection(cid, ratio):
    c2c, v2c = read_calib("calib_cam_to_cam.txt"), read_calib("calib_velo_to_cam.txt")
    P_rect = c2c["P_rect_" + cid].reshape(3, 4).copy()
    P_rect[0] *= T.WIDTH / T.RAW_W
    P_rect[1] *= T.HEIGHT / T.RAW_H
    return velo_projection(P_rect, c2c["R_rect_00"], v2c["R"], v2c["T"], ratio), P_rect


def golden_depth_inputs(ratio):
    """The fixtures' scans for cameras 02 and 03 in the order of the selected frames (2, 3, 6, 7 -> scan 0, 1, 0, 1):
    (points, scan_off, P [8, 3, 4], h, w, bounds, want [8, h, w])."""
    z = np.load(T.NPZ)
    scans = [z["scan0"], z["scan1"], z["scan0"], z["scan1"]] * 2
    P = np.stack([golden_projection(cid, ratio)[0] for cid in ("02", "03") for _ in range(4)])
    off = np.concatenate([[0], np.cumsum([len(s) for s in scans])]).astype(np.int32)
    h, w = T.HEIGHT // ratio, T.WIDTH // ratio
    want = z["depth_r%d" % ratio].reshape(8, h, w)
    return np.concatenate(scans), off, P, h, w, (T.WIDTH / ratio, T.HEIGHT / ratio), want


CLOUD_P = np.array([[240.0, 0, 200, 10], [0, 250.0, 60, 1], [0, 0, 1, 0.003]]) @ \
    np.array([[0.0, -1, 0, 0.0], [0, 0, -1, -0.08], [1, 0, 0, -0.27], [0, 0, 0, 1]])


def cloud(n, h, w, seed):
    """n points spread over (and around) an h x w map, some behind the sensor; P scaled to the map."""
    rng = np.random.default_rng(seed)
    pts = np.stack([rng.uniform(-5, 60, n), rng.uniform(-30, 30, n), rng.uniform(-3, 3, n), rng.uniform(0, 1, n)],
                   1).astype(np.float32)
    P = CLOUD_P.copy()
    P[0] *= w / 416
    P[1] *= h / 128
    return pts, P
