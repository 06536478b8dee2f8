"""The per-frame work of data/prepare_train_data.py on the GPU through libscsfm_prep.so (include/scsfm_prep.h).

    small = resize_u8(frames, 128, 416)                       # uint8 [N, H, W, C] -> [N, 128, 416, C], Pillow's bytes
    depth = velodyne_depth(points, scan_off, P, 128, 416, (416.0, 128.0))

Host side: Pillow's bilinear coefficient tables (ImagingResample: precompute_coeffs + normalize_coeffs_8bpc, for any
scale, with variable-length rows) and the velodyne-to-image matrix of KittiRawLoader.generate_depth_map in float64.
There is no CPU fallback: without a HIP device or the library the two wrappers raise.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _lib

PRECISION_BITS = 22  # Pillow: 32 - 8 - 2 (include/scsfm_prep.h: SCSFM_PREP_PRECISION_BITS)


def axis_table(in_size, out_size):
    """Pillow's bilinear taps for an axis resized in_size -> out_size: (rows int32 [out_size, 3] of first source index,
    tap count and offset of the first tap; taps int32 [sum of counts]).  None when the size does not change (Pillow
    skips that pass).  The support is max(in / out, 1): two or three taps when zooming in, 2 in / out + 1 when zooming
    out; the taps are normalised in double and rounded to 22-bit integers."""
    in_size, out_size = int(in_size), int(out_size)
    if in_size < 1 or out_size < 1:
        raise ValueError(f"cannot resize an axis of {in_size} to {out_size}")
    if in_size == out_size:
        return None
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support = 1.0 * filterscale  # the bilinear filter's support is 1
    ss = 1.0 / filterscale
    center = (np.arange(out_size) + 0.5) * scale
    xmin = np.maximum((center - support + 0.5).astype(np.int64), 0)
    xmax = np.minimum((center + support + 0.5).astype(np.int64), in_size)
    cnt = xmax - xmin
    kmax = int(cnt.max())
    k = np.zeros((out_size, kmax))
    ww = np.zeros(out_size)
    for i in range(kmax):
        x = np.abs((i + xmin - center + 0.5) * ss)
        w = np.where((i < cnt) & (x < 1.0), 1.0 - x, 0.0)
        k[:, i] = w
        ww = ww + w  # sequential double sum, as the C loop
    k = np.where(ww[:, None] != 0.0, k / np.where(ww == 0.0, 1.0, ww)[:, None], k)
    one = float(1 << PRECISION_BITS)
    ki = np.where(k < 0, (-0.5 + k * one).astype(np.int64), (0.5 + k * one).astype(np.int64))
    rows = np.zeros((out_size, 3), dtype=np.int32)
    rows[:, 0], rows[:, 1] = xmin, cnt
    rows[1:, 2] = np.cumsum(cnt)[:-1]
    taps = ki[np.arange(kmax)[None, :] < cnt[:, None]].astype(np.int32)  # row-major: each row's taps in order
    assert len(taps) == int(cnt.sum())
    return rows, taps


def resize_plan(H, W, height, width, keep_rows=None):
    """Everything scsfm_prep_resize_u8 needs beside the pixels: the two axis tables (None for a skipped pass), the
    kept rows and the range of source rows that the kept output rows reach."""
    keep = int(height) if keep_rows is None else int(keep_rows)
    if not 1 <= keep <= int(height):
        raise ValueError(f"keep_rows must be in [1, {height}], got {keep_rows}")
    htab, vtab = axis_table(W, width), axis_table(H, height)
    row0, rows = 0, int(H)
    if vtab is not None:
        vrows, vtaps = vtab
        vrows = vrows[:keep]
        n = int(vrows[-1, 2] + vrows[-1, 1])
        vtab = (np.ascontiguousarray(vrows), np.ascontiguousarray(vtaps[:n]))
        row0 = int(vrows[:, 0].min())
        rows = int((vrows[:, 0] + vrows[:, 1]).max()) - row0
    return dict(keep=keep, htab=htab, vtab=vtab, src_row0=row0, src_rows=rows)


def velo_projection(P_rect, R_rect_00, velo_R, velo_T, depth_size_ratio=1):
    """The velodyne -> image matrix as generate_depth_map forms it, in float64: the first two rows of a copy of P_rect
    divided by the ratio, times the 4x4 rectification, times the 4x4 velodyne-to-camera transform."""
    P = np.array(P_rect, dtype=np.float64).reshape(3, 4).copy()
    P[0] /= depth_size_ratio
    P[1] /= depth_size_ratio
    R = np.eye(4)
    R[:3, :3] = np.asarray(R_rect_00, dtype=np.float64).reshape(3, 3)
    V = np.hstack((np.asarray(velo_R, dtype=np.float64).reshape(3, 3), np.asarray(velo_T, dtype=np.float64)[..., np.newaxis]))
    V = np.vstack((V, np.array([0, 0, 0, 1.0])))
    return np.dot(np.dot(P, R), V)


def depth_map_size(img_height, img_width, depth_size_ratio):
    """(h, w, (bound_u, bound_v)) of a depth map; a ratio that does not divide the image size is rejected (the
    reference fails there with an index error on the first point of the last column or row)."""
    r = int(depth_size_ratio)
    if r < 1 or img_height % r or img_width % r:
        raise ValueError(f"depth_size_ratio {depth_size_ratio} does not divide {img_height} x {img_width}")
    return img_height // r, img_width // r, (img_width / r, img_height / r)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _check_device(t, what):
    if not torch.cuda.is_available() or not t.is_cuda:
        raise RuntimeError(f"{what} must live on a HIP device (there is no CPU fallback)")


def _stream(t):
    return ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def resize_u8(images, height, width, keep_rows=None):
    """uint8 [N, H, W, C] on the device (C in {1, 3, 4}) -> uint8 [N, keep_rows, width, C]: the first keep_rows
    (default: all) rows of Pillow's ``Image.resize((width, height), BILINEAR)`` of every frame, byte for byte.  The
    channels are resampled independently (Pillow premultiplies RGBA by its alpha first; this does not)."""
    _check_device(images, "images")
    if images.dtype != torch.uint8 or images.dim() != 4 or images.shape[3] not in (1, 3, 4) or images.shape[0] < 1:
        raise ValueError("images must be uint8 [N, H, W, C] with N >= 1 and C in {1, 3, 4}")
    images = images.contiguous()
    N, H, W, C = images.shape
    plan = resize_plan(H, W, height, width, keep_rows)
    dev = images.device
    lib = _lib.get_prep()

    def up(tab):
        if tab is None:
            return None, None, 0
        return torch.from_numpy(tab[0]).to(dev), torch.from_numpy(tab[1]).to(dev), len(tab[1])

    hrows, htaps, nh = up(plan["htab"])
    vrows, vtaps, nv = up(plan["vtab"])
    both = hrows is not None and vrows is not None
    nbytes = lib.size("scsfm_prep_resize_workspace_bytes", N, C, int(width), plan["src_rows"], int(both))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev) if nbytes else None
    out = torch.empty((N, plan["keep"], int(width), C), dtype=torch.uint8, device=dev)
    lib.call("scsfm_prep_resize_u8", N, H, W, C, plan["keep"], int(width), _ptr(images), _ptr(hrows), _ptr(htaps), nh,
             _ptr(vrows), _ptr(vtaps), nv, plan["src_row0"], plan["src_rows"], _ptr(out), _ptr(ws), nbytes,
             _stream(images))
    return out


def velodyne_depth(points, scan_off, P, height, width, bounds):
    """generate_depth_map for F scans in one call.  ``points`` float32 [total, 4] (forward, left, up, reflectance),
    ``scan_off`` int32 [F + 1], ``P`` float64 [F, 3, 4] (velo_projection), all on the device; ``bounds`` the real
    (img_width / ratio, img_height / ratio) -> float32 [F, height, width]."""
    _check_device(points, "points")
    if points.dtype != torch.float32 or points.dim() != 2 or points.shape[1] != 4:
        raise ValueError("points must be float32 [total, 4]")
    if scan_off.dtype != torch.int32 or scan_off.dim() != 1 or len(scan_off) < 2:
        raise ValueError("scan_off must be int32 [F + 1]")
    F = len(scan_off) - 1
    if P.dtype != torch.float64 or tuple(P.shape) != (F, 3, 4):
        raise ValueError(f"P must be float64 [{F}, 3, 4]")
    h, w = int(height), int(width)
    bu, bv = float(bounds[0]), float(bounds[1])
    if not (0 < bu <= w and 0 < bv <= h):
        raise ValueError(f"bounds {bounds} do not fit a {h} x {w} map")
    dev = points.device
    points, scan_off, P = points.contiguous(), scan_off.to(dev).contiguous(), P.to(dev).contiguous()
    lib = _lib.get_prep()
    nbytes = lib.size("scsfm_prep_velo_workspace_bytes", F, h, w)
    if nbytes == 0:
        raise ValueError(f"{F} depth maps of {h} x {w} are more than one call takes")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    depth = torch.empty((F, h, w), dtype=torch.float32, device=dev)
    lib.call("scsfm_prep_velo_depth", F, h, w, bu, bv, _ptr(points) if len(points) else None, len(points),
             _ptr(scan_off), _ptr(P), _ptr(depth), _ptr(ws), nbytes, _stream(points))
    return depth
