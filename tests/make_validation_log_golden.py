"""Writes tests/golden/validation_log.npz: small maps, an input batch and a ground-truth depth, and what the reference's
own tensor2array and validate_with_gt, called through tests/_validation_log_ref.py, make of them as float arrays, with
its three float tables.

    python tests/make_validation_log_golden.py          (needs the reference and matplotlib)
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.join(os.path.dirname(HERE), "sc-sfmlearner-release_amd")]

import _inference_vis_cases as C  # noqa: E402
import _validation_log_golden as G  # noqa: E402
import _validation_log_ref as R  # noqa: E402

OUT = G.PATH
CALLS = G.CALLS


def maps_a():
    """Six 9 x 13 maps (117 pixels: images 1 to 5 start off a 16-byte boundary): plain; the maximum last and a negative
    value; +0 and -0; a NaN; all zero; one holding +inf."""
    m = C.base((6, 9, 13), seed=11)
    m[1, -1, -1] = m[1].max() * np.float32(1.5)
    m[1, 2, 3] = -0.25
    m[2, 5, 7], m[2, 0, 0] = 0.0, -0.0
    m[3, 4, 11] = np.nan
    m[4] = 0.0
    m[5, 3, 3] = np.inf
    return m


def maps_b():
    """Two aligned 8 x 16 maps; the second holds, for max_value = 10, pixels at exactly 10, just above, far above and
    below zero."""
    m = C.base((2, 8, 16), seed=12)
    m[1] *= np.float32(4)
    m[1, 1, 2] = 10.0
    m[1, 2, 3] = np.float32(10.000001)
    m[1, 7, 15] = 12.5
    m[1, 0, 0] = -1.0
    m[1, 4, 4] = np.float32(9.999999)
    return m


def maps_c():
    return np.full((1, 1, 1), 0.37, np.float32)


def batch():
    """float32 [2, 3, 5, 11]: every byte value k as the normalised input (k / 255 - 0.45) / 0.225 (330 values, the torch
    CPU expression), plus values the bytes clamp: below 0, above 1 and a NaN."""
    import torch
    k = torch.from_numpy((np.arange(330) % 256).astype(np.float32))
    x = ((k / 255 - 0.45) / 0.225).numpy().reshape(2, 3, 5, 11).copy()
    x[1, 2, 4, 8:] = [-2.5, 3.0, np.nan]
    return x


def gt_depth():
    """float32 [2, 9, 13]: zeros of both signs, values below 0.1 (a disparity above 10), a negative; image 1 holds a NaN
    and +inf as well."""
    rng = np.random.default_rng(13)
    d = rng.uniform(0.5, 80.0, (2, 9, 13)).astype(np.float32)
    d[rng.random(d.shape) < 0.3] = 0.0
    d[0, 0, 0], d[0, 0, 1], d[0, 1, 1], d[0, 2, 2], d[0, 8, 12] = -0.0, 0.05, 0.0999, -3.0, 0.1
    d[1, 3, 3], d[1, 4, 4], d[1, 5, 5] = np.nan, np.inf, 0.02
    return d


def main():
    assert R.available(), "the reference and matplotlib are needed"
    out = {name: R.float_table(name) for name in R.NAMES}
    for key, maps in (("a", maps_a()), ("b", maps_b()), ("c", maps_c())):
        out[f"maps_{key}"] = maps
        for cmap, max_value in CALLS:
            out[f"{key}/{cmap}"] = R.map_pictures(maps, max_value, cmap)
    out["batch"] = batch()
    out["batch/floats"] = R.input_pictures(out["batch"])
    out["gt"] = gt_depth()
    out["gt/depth_picture"], out["gt/disparity"], out["gt/disparity_picture"] = R.target(out["gt"])
    out["bone_bit_steps"] = G.bit_steps(out.pop("bone"))
    assert np.array_equal(G.from_bit_steps(out["bone_bit_steps"]), R.float_table("bone"))
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
