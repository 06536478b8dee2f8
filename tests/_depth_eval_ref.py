"""Runs the reference's own evaluation code (eval_depth.py: compute_depth_errors and DepthEvalEigen.evaluate_depth),
pulled out of its source with ``ast`` -- the module itself parses argv and evaluates at import -- in a namespace that
holds real numpy, the ``args`` it reads and a cv2 whose ``resize`` is the oracle's INTER_LINEAR.  It records what
reaches compute_depth_errors (the masked, scaled and clamped pairs), the errors, the ratios and the printout."""
from __future__ import annotations

import ast
import contextlib
import io
import os
import types
import warnings

import numpy as np

import depth_eval_oracle as O

REFERENCE = os.environ.get("SCSFM_REFERENCE", "/root/reference")
EVAL_DEPTH = os.path.join(REFERENCE, "eval_depth.py")


def available():
    return os.path.isfile(EVAL_DEPTH)


def _extract():
    tree = ast.parse(open(EVAL_DEPTH).read())
    keep = [n for n in tree.body if isinstance(n, (ast.FunctionDef, ast.ClassDef))
            and n.name in ("compute_depth_errors", "DepthEvalEigen")]
    return compile(ast.Module(body=keep, type_ignores=[]), EVAL_DEPTH, "exec")


def run(gt_depths, pred_depths, dataset):
    """-> dict(pairs=[(gt, pred)], errors=[tuple], ratios=array, stdout=str)"""
    rec = dict(pairs=[], errors=[], ratios=None)

    class NP(types.SimpleNamespace):
        def __getattr__(self, name):
            return getattr(np, name)

    def savetxt(name, arr, fmt):
        rec["ratios"] = np.array(arr)

    ns = dict(np=NP(savetxt=savetxt), tqdm=lambda x: x,
              cv2=types.SimpleNamespace(resize=lambda src, dsize: O.resize_linear(src, dsize[0], dsize[1])),
              args=types.SimpleNamespace(dataset=dataset, ratio_name="ratios.txt", vis_dir=None))
    exec(_extract(), ns)
    errors = ns["compute_depth_errors"]

    def recording(gt, pred):
        rec["pairs"].append((gt.copy(), pred.copy()))
        e = errors(gt, pred)
        rec["errors"].append(e)
        return e

    ns["compute_depth_errors"] = recording
    out = io.StringIO()
    with contextlib.redirect_stdout(out), warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        ns["DepthEvalEigen"]().evaluate_depth(gt_depths, pred_depths, eval_mono=True)
    rec["stdout"] = out.getvalue()
    return rec
