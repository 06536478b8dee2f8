"""Writes tests/golden/inference_vis.npz: a handful of small disparity maps and what the reference's own utils.py
(tests/_inference_vis_ref.py) makes of them, its two byte tables, and the flags of its run_inference.py.

    python tests/make_inference_vis_golden.py          (needs the reference and matplotlib)
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.join(os.path.dirname(HERE), "sc-sfmlearner-release_amd")]

import _inference_vis_cases as C  # noqa: E402
import _inference_vis_ref as R  # noqa: E402

OUT = os.path.join(HERE, "golden", "inference_vis.npz")
SHAPE = (6, 24, 31)


def inputs():
    """Six maps: plain; the maximum last and a negative value; +0 and -0; a NaN; all zero; mostly farther than 10."""
    m = C.base(SHAPE, seed=7)
    m[1, -1, -1] = m[1].max() * np.float32(1.5)
    m[1, 2, 3] = -0.25
    m[2, 5, 7], m[2, 0, 0] = 0.0, -0.0
    m[3, 11, 13] = np.nan
    m[4] = 0.0
    m[5] *= np.float32(0.12)
    return m


def main():
    assert R.available(), "the reference and matplotlib are needed"
    disp = inputs()
    pics = [R.pictures(d[None]) for d in disp]
    np.savez_compressed(OUT, disp=disp, disp_pictures=np.stack([p[0] for p in pics]),
                        depth_pictures=np.stack([p[1] for p in pics]), bone=R.byte_table("bone"),
                        rainbow=R.byte_table("rainbow"), parser=np.array(json.dumps(R.parser_spec())))
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
