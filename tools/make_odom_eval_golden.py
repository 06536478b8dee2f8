"""Writes tests/golden/odom_eval.npz: the ground-truth poses of KITTI odometry sequences 04 and 10, a predicted
trajectory for each, and what the reference's own KittiEvalOdom (run through tests/_odom_eval_ref.py) records on them
for each of its five alignment modes: the segment table, the five summary numbers, result.txt and the printout (and
errors/NN.txt for one mode).  The GPU tests replay the file without the reference.

The prediction is what test_vo.py would write for a network that is nearly right: the GT's relative motions with a
monocular scale and seeded noise, as float32 pose vectors, pose_vec2mat in float32, folded in float64 and rounded
through '%1.8e'.

    python tools/make_odom_eval_golden.py
"""
import io
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "sc-sfmlearner-release_amd")]

import _odom_eval_ref as REF  # noqa: E402
import odom_eval_oracle as O  # noqa: E402

SEQS = (4, 10)
SCALE = 0.031
NAMES = {None: "none", "scale": "scale", "scale_7dof": "scale_7dof", "7dof": "7dof", "6dof": "6dof"}


def pose_vectors(gt, seed):
    """float32 [n - 1, 6]: vector k describes inv(inv(G_k) G_k+1) (test_vo.py folds the inverses), euler angles of
    R = Rx Ry Rz, the translation scaled, both with noise."""
    g = O.split(gt)
    rel = O.amul(O.ainv(O.sel(g, slice(0, -1))), O.sel(g, slice(1, None)))
    R, t = O.ainv(rel)
    rng = np.random.default_rng(seed)
    ang = np.stack([np.arctan2(-R[:, 1, 2], R[:, 2, 2]), np.arcsin(np.clip(R[:, 0, 2], -1, 1)),
                    np.arctan2(-R[:, 0, 1], R[:, 0, 0])], 1)
    ang = ang + rng.normal(0.0, 4e-4, ang.shape) + 3e-5
    t = t * SCALE * (1.0 + rng.normal(0.0, 0.03, (len(t), 1))) + rng.normal(0.0, 2e-4, t.shape)
    return np.concatenate([t, ang], 1).astype(np.float32)


def trajectories():
    """-> (gts, preds): lists of [n, 12] float64 for SEQS."""
    gts, preds = [], []
    for seq in SEQS:
        gt = np.loadtxt(REF.gt_path(seq)).reshape(-1, 12)
        poses = O.fold(O.euler_mat(pose_vectors(gt, seed=100 + seq)))
        buf = io.StringIO()
        REF.write_poses(buf, poses)
        gts.append(gt)
        preds.append(np.loadtxt(io.StringIO(buf.getvalue())).reshape(-1, 12))
    return gts, preds


def main():
    if not REF.available():
        raise SystemExit(f"the reference is needed: {REF.MODULE}")
    gts, preds = trajectories()
    data = dict(seqs=np.array(SEQS))
    for seq, g, p in zip(SEQS, gts, preds):
        data[f"gt_{seq:02}"], data[f"pred_{seq:02}"] = g, p
    for alignment, name in NAMES.items():
        rec = REF.run(gts, preds, SEQS, alignment)
        for seq, seg in zip(SEQS, rec["seg"]):
            data[f"seg_{name}_{seq:02}"] = seg
        data[f"summary_{name}"] = rec["summary"]
        data[f"result_{name}"] = np.array(rec["result_txt"])
        data[f"stdout_{name}"] = np.array(rec["stdout"])
        if alignment == "7dof":
            for seq, text in zip(SEQS, rec["errors"]):
                data[f"errors_{name}_{seq:02}"] = np.array(text)
    path = os.path.join(ROOT, "tests", "golden", "odom_eval.npz")
    np.savez_compressed(path, **data)
    print(path, os.path.getsize(path))


if __name__ == "__main__":
    main()
