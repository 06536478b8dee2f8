"""Writes tests/golden/depth_eval_{kitti,nyu}.npz: small synthetic evaluation sets (tests/_depth_eval_data.py) with what
the reference's own evaluation code (eval_depth.py, run through tests/_depth_eval_ref.py) computes on them: per-image
errors in its column order, the ratios and the printout.  The GPU tests replay them without the reference.

    python tools/make_depth_eval_golden.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "sc-sfmlearner-release_amd")]

import _depth_eval_data as D  # noqa: E402
import _depth_eval_ref as REF  # noqa: E402


def sets():
    """The fixtures' inputs: a ragged KITTI-like set with float64 predictions (one of them skipped) and
    a dense NYU-like set with float32 predictions."""
    gts, pred = D.kitti_set(6, seed=11, sizes=((47, 156), (46, 153), (47, 155), (48, 157)), pred_hw=(16, 52),
                            density=0.25)
    pred[2] = -1.0
    ngt, npred = D.nyu_set(5, seed=12, gt_hw=(48, 64), pred_hw=(26, 32), pred_dtype=np.float32)
    return {"kitti": (gts, pred), "nyu": (ngt, npred)}


def main():
    if not REF.available():
        raise SystemExit(f"the reference is needed: {REF.EVAL_DEPTH}")
    for name, (gts, pred) in sets().items():
        rec = REF.run(gts, pred, name)
        path = os.path.join(ROOT, "tests", "golden", f"depth_eval_{name}.npz")
        np.savez_compressed(path, gt=np.concatenate([g.ravel() for g in gts]),
                            gt_shapes=np.array([g.shape for g in gts]), pred=pred, errors=np.array(rec["errors"]),
                            ratios=rec["ratios"], stdout=np.array(rec["stdout"]))
        print(path, os.path.getsize(path))


if __name__ == "__main__":
    main()
