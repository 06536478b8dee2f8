"""Runs the reference's own KittiEvalOdom (kitti_eval/kitti_odometry.py) on pose files written to a temporary directory,
with matplotlib replaced by an empty stand-in while the module is imported and the two plotting methods stubbed out.  It
records the per-segment errors and the five summary numbers as the reference holds them, result.txt, errors/NN.txt and
the printout."""
from __future__ import annotations

import contextlib
import importlib.util
import io
import os
import sys
import tempfile
import types
import warnings

import numpy as np

REFERENCE = os.environ.get("SCSFM_REFERENCE", "/root/reference")
MODULE = os.path.join(REFERENCE, "kitti_eval", "kitti_odometry.py")


def available():
    return os.path.isfile(MODULE)


def gt_path(seq):
    return os.path.join(REFERENCE, "kitti_eval", "gt_poses", "{:02}.txt".format(seq))


def _module():
    saved = {k: sys.modules.get(k) for k in ("matplotlib", "matplotlib.pyplot")}
    mpl = types.ModuleType("matplotlib")
    mpl.pyplot = types.ModuleType("matplotlib.pyplot")
    sys.modules["matplotlib"], sys.modules["matplotlib.pyplot"] = mpl, mpl.pyplot
    try:
        spec = importlib.util.spec_from_file_location("_reference_kitti_odometry", MODULE)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    return mod


def write_poses(path, poses):
    """KITTI's text format as test_vo.py writes it."""
    np.savetxt(path, np.reshape(poses, (-1, 12)), delimiter=' ', fmt='%1.8e')


def run(gts, preds, seqs, alignment=None):
    """gts / preds: lists of [n, 12] arrays, written out as NN.txt (GT with full precision, predictions as given) ->
    dict(seg=[per sequence [m, 5]], summary=[S, 5] (ave_t, ave_r, ate, rpe_t, rpe_r), result_txt, stdout,
    errors=[per sequence text])."""
    mod = _module()
    rec = dict(seg=[], summary=[])

    class Eval(mod.KittiEvalOdom):
        def plot_trajectory(self, *a):
            pass

        def plot_error(self, *a):
            pass

        def calc_sequence_errors(self, poses_gt, poses_result):
            err = super().calc_sequence_errors(poses_gt, poses_result)
            rec["seg"].append(np.array(err, np.float64).reshape(-1, 5))
            return err

        def write_result(self, f, seq, errs):
            rec["summary"].append([float(e) for e in errs])
            return super().write_result(f, seq, errs)

    with tempfile.TemporaryDirectory() as tmp:
        gt_dir, res_dir = os.path.join(tmp, "gt"), os.path.join(tmp, "res")
        os.makedirs(gt_dir), os.makedirs(res_dir)
        for seq, g, p in zip(seqs, gts, preds):
            np.savetxt(os.path.join(gt_dir, "{:02}.txt".format(seq)), np.reshape(g, (-1, 12)), delimiter=' ', fmt='%.17e')
            np.savetxt(os.path.join(res_dir, "{:02}.txt".format(seq)), np.reshape(p, (-1, 12)), delimiter=' ', fmt='%.17e')
        out = io.StringIO()
        with contextlib.redirect_stdout(out), warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            Eval().eval(gt_dir, res_dir, alignment=alignment, seqs=list(seqs))
        rec["stdout"] = out.getvalue()
        rec["result_txt"] = open(os.path.join(res_dir, "result.txt")).read()
        rec["errors"] = [open(os.path.join(res_dir, "errors", "{:02}.txt".format(s))).read() for s in seqs]
    rec["summary"] = np.array(rec["summary"], np.float64).reshape(-1, 5)
    return rec
