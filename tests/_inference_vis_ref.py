"""Runs the reference's own utils.py (tensor2array, opencv_rainbow, COLORMAPS) and reads run_inference.py's parser on a
current stack.  utils.py is imported with ``path`` replaced by a small str subclass and with ``matplotlib.cm.get_cmap``,
which current matplotlib no longer has, given back for the duration of the import as
``matplotlib.colormaps[name]`` (``.resampled(lutsize)`` when a size is asked for).  Nothing of the reference is kept
here: it is loaded from its own files when a test runs, and the tests skip when it or matplotlib is absent."""
from __future__ import annotations

import ast
import importlib.util
import os
import sys
import types

import numpy as np

REFERENCE = os.environ.get("SCSFM_REFERENCE", "/root/reference")
UTILS = os.path.join(REFERENCE, "utils.py")
CLI = os.path.join(REFERENCE, "run_inference.py")


def available():
    if not (os.path.isfile(UTILS) and os.path.isfile(CLI)):
        return False
    try:
        import matplotlib  # noqa: F401
    except ImportError:
        return False
    return True


class Path(str):
    def __truediv__(self, other):
        return Path(os.path.join(self, other))


def _get_cmap(name, lutsize=None):
    import matplotlib
    cmap = matplotlib.colormaps[name]
    return cmap if lutsize is None else cmap.resampled(lutsize)


_utils = None


def utils():
    """The reference's utils module."""
    global _utils
    if _utils is None:
        from matplotlib import cm
        stub = types.ModuleType("path")
        stub.Path = Path
        saved_path = sys.modules.get("path")
        saved_get = cm.__dict__.get("get_cmap")
        sys.modules["path"] = stub
        cm.get_cmap = _get_cmap
        try:
            spec = importlib.util.spec_from_file_location("_reference_utils", UTILS)
            mod = importlib.util.module_from_spec(spec)
            spec.loader.exec_module(mod)
        finally:
            if saved_path is None:
                sys.modules.pop("path", None)
            else:
                sys.modules["path"] = saved_path
            if saved_get is None:
                del cm.get_cmap
            else:
                cm.get_cmap = saved_get
        _utils = mod
    return _utils


def byte_table(name):
    """uint8 [N, 4]: the reference's colour map ``name`` at each of its N entries, as run_inference.py turns colours
    into bytes."""
    cmap = utils().COLORMAPS[name]
    rgba = cmap(np.arange(cmap.N))  # integer input: the entries themselves
    return (255 * rgba.astype(np.float32)).astype(np.uint8)


def pictures(disp):
    """run_inference.py's two pictures for one disparity map, float32 [1, H, W] -> (uint8 [H, W, 4], uint8 [H, W, 4]),
    with its own statements around tensor2array."""
    import torch
    U = utils()
    output = torch.from_numpy(np.ascontiguousarray(disp, dtype=np.float32))
    with np.errstate(all="ignore"):
        d = (255 * U.tensor2array(output, max_value=None, colormap='bone')).astype(np.uint8)
        depth = 1 / output
        z = (255 * U.tensor2array(depth, max_value=10, colormap='rainbow')).astype(np.uint8)
    return np.transpose(d, (1, 2, 0)), np.transpose(z, (1, 2, 0))


def parser_spec():
    """[(flag, default, action-or-None, help)] of every add_argument call of the reference's run_inference.py, read from
    its syntax tree (the script itself imports modules that no longer exist)."""
    tree = ast.parse(open(CLI).read())
    out = []
    for node in ast.walk(tree):
        if isinstance(node, ast.Call) and getattr(node.func, "attr", None) == "add_argument":
            kw = {k.arg: ast.literal_eval(k.value) for k in node.keywords if k.arg in ("default", "action", "help", "required")}
            out.append([ast.literal_eval(node.args[0]), kw.get("default"), kw.get("action"), kw.get("help"),
                        bool(kw.get("required", False))])
    return out
