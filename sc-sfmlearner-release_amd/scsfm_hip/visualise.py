"""The per-image work of run_inference.py on the GPU through libscsfm_vis.so (include/scsfm_vis.h).

    x = normalise_u8(frames)                                  # uint8 [N, H, W, 3] -> float32 [N, 3, H, W]
    disp_rgba, depth_rgba = disparity_and_depth_images(disp)  # uint8 [N, H, W, 4] each, on the device

``colourise`` is the reference's ``(255 * tensor2array(t, max_value, colormap)).astype(np.uint8)`` byte for byte, with
matplotlib's under / over / bad rules: 'bone' with 10 000 entries for disparities, the OpenCV-style 'rainbow' with 1000
for depths.  Host side: the two byte tables, built in numpy from the colour maps' segment data (no matplotlib) and kept
on each device after the first use.  There is no CPU fallback: without a HIP device or the library the wrappers raise.
"""
from __future__ import annotations

import ctypes
import functools

import numpy as np
import torch

from . import _lib

# matplotlib's `bone` (cm._bone_data): per channel the stops (x, y)
_BONE = {
    "red": ((0., 0.), (0.746032, 0.652778), (1.0, 1.0)),
    "green": ((0., 0.), (0.365079, 0.319444), (0.746032, 0.777778), (1.0, 1.0)),
    "blue": ((0., 0.), (0.365079, 0.444444), (1.0, 1.0)),
}
# the OpenCV equivalent of rainbow: (x, (r, g, b))
_RAINBOW = ((0.000, (1.00, 0.00, 0.00)), (0.400, (1.00, 1.00, 0.00)), (0.600, (0.00, 1.00, 0.00)),
            (0.800, (0.00, 0.00, 1.00)), (1.000, (0.60, 0.00, 1.00)))
_SEGMENTS = {
    "bone": (10000, _BONE),
    "rainbow": (1000, {c: tuple((x, rgb[i]) for x, rgb in _RAINBOW) for i, c in enumerate(("red", "green", "blue"))}),
}


def _channel(n, stops):
    """A linear-segmented channel sampled at linspace(0, 1, n), as matplotlib's _create_lookup_table forms it (float64;
    the stops are continuous, y0 == y1)."""
    x = np.array([s[0] for s in stops], dtype=np.float64)
    y = np.array([s[1] for s in stops], dtype=np.float64)
    xind = np.linspace(0.0, 1.0, n)
    ind = np.searchsorted(x, xind)[1:-1]
    dist = (xind[1:-1] - x[ind - 1]) / (x[ind] - x[ind - 1])
    lut = np.concatenate([[y[0]], dist * (y[ind] - y[ind - 1]) + y[ind - 1], [y[-1]]])
    return np.clip(lut, 0.0, 1.0)


@functools.lru_cache(maxsize=None)
def colour_table(name):
    """uint8 [N, 4]: uint8(float32(255) * float32(rgba)) of every entry of the colour map: 'bone' (N = 10 000) or
    'rainbow' (N = 1000).  Read-only; any other name raises ValueError."""
    if name not in _SEGMENTS:
        raise ValueError(f"unknown colour map {name!r} (known: {sorted(_SEGMENTS)})")
    n, seg = _SEGMENTS[name]
    rgba = np.stack([_channel(n, seg[c]) for c in ("red", "green", "blue")] + [np.ones(n)], axis=1)
    table = (np.float32(255) * rgba.astype(np.float32)).astype(np.uint8)
    table.setflags(write=False)
    return table


_device_tables = {}


def _table_on(name, device):
    key = (name, device.index if device.index is not None else torch.cuda.current_device())
    if key not in _device_tables:
        _device_tables[key] = torch.from_numpy(colour_table(name).copy()).to(device)
    return _device_tables[key]


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _check_device(t, what):
    if not torch.cuda.is_available() or not t.is_cuda:
        raise RuntimeError(f"{what} must live on a HIP device (there is no CPU fallback)")


def _stream(t):
    return ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def normalise_u8(frames):
    """uint8 [N, H, W, 3] on the device -> float32 [N, 3, H, W]: (x / 255 - 0.45) / 0.225, the bits of the torch CPU
    expression."""
    _check_device(frames, "frames")
    if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[3] != 3 or frames.numel() < 1:
        raise ValueError("frames must be uint8 [N, H, W, 3] with at least one pixel")
    frames = frames.contiguous()
    N, H, W, _ = frames.shape
    with torch.cuda.device(frames.device):
        out = torch.empty((N, 3, H, W), dtype=torch.float32, device=frames.device)
        _lib.get_vis().call("scsfm_vis_normalise_u8", N, H, W, _ptr(frames), _ptr(out), _stream(frames))
    return out


def _maps(maps):
    _check_device(maps, "maps")
    if maps.dtype != torch.float32 or maps.dim() != 3 or maps.numel() < 1:
        raise ValueError("maps must be float32 [N, H, W] with at least one pixel")
    return maps.contiguous()


def image_max(maps):
    """float32 [N, H, W] on the device -> float32 [N]: every image's maximum, NaN when the image holds one."""
    maps = _maps(maps)
    N, H, W = maps.shape
    with torch.cuda.device(maps.device):
        out = torch.empty(N, dtype=torch.float32, device=maps.device)
        _lib.get_vis().call("scsfm_vis_image_max", N, H * W, _ptr(maps), _ptr(out), _stream(maps))
    return out


def colourise(maps, colormap='rainbow', max_value=None, reciprocal=False):
    """float32 [N, H, W] on the device -> uint8 [N, H, W, 4] on the device: the reference's
    ``255 * tensor2array(map, max_value, colormap)`` as bytes, per image.  ``max_value=None`` divides every image by
    its own maximum (found on the device, no host round trip); ``reciprocal`` colours 1 / map and needs a
    ``max_value``."""
    table = colour_table(colormap)
    if reciprocal and max_value is None:
        raise ValueError("a reciprocal picture needs a max_value")
    maps = _maps(maps)
    N, H, W = maps.shape
    with torch.cuda.device(maps.device):
        divisors = image_max(maps) if max_value is None else None
        dev_table = _table_on(colormap, maps.device)
        out = torch.empty((N, H, W, 4), dtype=torch.uint8, device=maps.device)
        _lib.get_vis().call("scsfm_vis_colourise", N, H, W, _ptr(maps), _ptr(dev_table), len(table), _ptr(divisors),
                            0.0 if max_value is None else float(max_value), int(bool(reciprocal)), _ptr(out),
                            _stream(maps))
    return out


def disparity_and_depth_images(disp):
    """Both pictures of run_inference.py for a batch of disparities, float32 [N, 1, H, W] or [N, H, W]: (bone over
    disp / max(disp), rainbow over (1 / disp) / 10), uint8 [N, H, W, 4] each."""
    if disp.dim() == 4:
        if disp.shape[1] != 1:
            raise ValueError("disp must be [N, 1, H, W] or [N, H, W]")
        disp = disp[:, 0]
    return (colourise(disp, colormap='bone', max_value=None),
            colourise(disp, colormap='rainbow', max_value=10, reciprocal=True))
