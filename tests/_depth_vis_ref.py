"""Runs the reference's own visualisation code (eval_depth.py: depth_visualizer, depth_pair_visualizer and
DepthEvalEigen.evaluate_depth's return value), pulled out of its source with ``ast`` as tests/_depth_eval_ref.py does --
the module itself parses argv, imports OpenCV and evaluates at import.  Nothing of it is kept."""
from __future__ import annotations

import ast
import contextlib
import io
import os
import types
import warnings

import numpy as np

import depth_eval_oracle as E

REFERENCE = os.environ.get("SCSFM_REFERENCE", "/root/reference")
EVAL_DEPTH = os.path.join(REFERENCE, "eval_depth.py")
NAMES = ("compute_depth_errors", "depth_visualizer", "depth_pair_visualizer", "DepthEvalEigen")


def available():
    if not os.path.isfile(EVAL_DEPTH):
        return False
    try:
        import matplotlib  # noqa: F401
    except ImportError:
        return False
    return True


def namespace(dataset):
    import matplotlib as mpl
    import matplotlib.cm as cm
    tree = ast.parse(open(EVAL_DEPTH).read())
    keep = [n for n in tree.body if isinstance(n, (ast.FunctionDef, ast.ClassDef)) and n.name in NAMES]
    ns = dict(np=np, mpl=mpl, cm=cm, tqdm=lambda x: x,
              cv2=types.SimpleNamespace(resize=lambda src, dsize: E.resize_linear(src, dsize[0], dsize[1])),
              args=types.SimpleNamespace(dataset=dataset, ratio_name=None, vis_dir=None))
    exec(compile(ast.Module(body=keep, type_ignores=[]), EVAL_DEPTH, "exec"), ns)
    return ns


def quiet(fn, *args):
    with contextlib.redirect_stdout(io.StringIO()), warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        return fn(*args)


def depth_visualizer(x):
    return quiet(namespace("kitti")["depth_visualizer"], x)


def depth_pair_visualizer(pred, gt):
    return quiet(namespace("nyu")["depth_pair_visualizer"], pred, gt)


def resized_predictions(gt_depths, pred_depths, dataset):
    """What evaluate_depth returns: the scaled predictions of the evaluated images."""
    return quiet(namespace(dataset)["DepthEvalEigen"]().evaluate_depth, gt_depths, pred_depths, True)


def magma_table():
    import matplotlib as mpl
    return (np.array(mpl.colormaps["magma"].colors, dtype=np.float64) * 255).astype(np.uint8)
