"""Compiles the visualisation kernels (sc-sfmlearner-release_amd/csrc_vis/*.hip), unchanged, against the host simulator
(tests/hostsim/hip/hip_runtime.h) with g++ into tests/hostsim/_build_vis/, and runs the C ABI of include/scsfm_vis.h on
HOST pointers.  Test infrastructure only; never loaded by the product."""
from __future__ import annotations

import ctypes
import functools
import os

import numpy as np

from hostsim import library
from scsfm_hip import visualise
from scsfm_hip._lib import VIS_ABI_VERSION, VIS_HEADER, CLib

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(ROOT, "sc-sfmlearner-release_amd", "csrc_vis")
HOSTSIM = os.path.join(HERE, "hostsim")
OUT = os.path.join(HOSTSIM, "_build_vis")
LIB = os.path.join(OUT, "libscsfm_vis_hostsim.so")


def build(force=False):
    return library.build("vis", force, dep=os.path.abspath(__file__))


@functools.lru_cache(maxsize=1)
def lib():
    return CLib(build(), VIS_HEADER, VIS_ABI_VERSION, "scsfm_vis_")


def _ptr(a):
    return ctypes.c_void_p(a.ctypes.data) if a is not None else None


def _aligned(shape, dtype, fill, offset=0):
    """An array whose first byte sits ``offset`` bytes past a 64-byte boundary, every byte ``fill``."""
    n = int(np.prod(shape)) * np.dtype(dtype).itemsize
    raw = np.full(n + 128, fill, np.uint8)
    start = (-raw.ctypes.data) % 64 + offset
    return raw[start:start + n].view(dtype).reshape(shape)


def normalise_u8(frames):
    """scsfm_hip.visualise.normalise_u8 on the simulator.  The output starts as 0xAB bytes."""
    frames = np.ascontiguousarray(frames, np.uint8)
    N, H, W, _ = frames.shape
    out = _aligned((N, 3, H, W), np.float32, 0xAB)
    lib().call("scsfm_vis_normalise_u8", N, H, W, _ptr(frames), _ptr(out), None)
    return out


def image_max(maps):
    maps = np.ascontiguousarray(maps, np.float32)
    N, H, W = maps.shape
    out = _aligned((N,), np.float32, 0xAB)
    lib().call("scsfm_vis_image_max", N, H * W, _ptr(maps), _ptr(out), None)
    return out


def colourise(maps, colormap="rainbow", max_value=None, reciprocal=False, offset=0):
    """scsfm_hip.visualise.colourise on the simulator, numpy in and out.  The output starts as 0xAB bytes.  ``offset``
    (a multiple of 4) moves both buffers off the 16-byte boundary, which takes the one-pixel-per-lane path only."""
    table = np.ascontiguousarray(visualise.colour_table(colormap))
    N, H, W = maps.shape
    src = _aligned((N, H, W), np.float32, 0, offset)
    src[...] = maps
    divisors = image_max(src) if max_value is None else None
    out = _aligned((N, H, W, 4), np.uint8, 0xAB, offset)
    lib().call("scsfm_vis_colourise", N, H, W, _ptr(src), _ptr(table), len(table), _ptr(divisors),
               0.0 if max_value is None else float(max_value), int(bool(reciprocal)), _ptr(out), None)
    return out
