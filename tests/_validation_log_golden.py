"""Reads tests/golden/validation_log.npz (written by tests/make_validation_log_golden.py).  The 10 000-entry bone table
is kept as the steps between the bit patterns of consecutive entries (float32 ramps do not compress, their steps do:
4 kB instead of 92 kB); ``load()`` puts the table back, bit for bit."""
import os

import numpy as np

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "validation_log.npz")
# (colormap, max_value) of the recorded pictures: the two train.py makes, and bone for the third table
CALLS = (("magma", None), ("rainbow", 10), ("bone", None))


def bit_steps(table):
    return np.diff(np.ascontiguousarray(table, np.float32).view(np.uint32).astype(np.int64), axis=0, prepend=0)


def from_bit_steps(steps):
    return np.ascontiguousarray(np.cumsum(steps, axis=0).astype(np.uint32)).view(np.float32)


_golden = None


def load():
    """{name: array}; read once, the arrays read-only."""
    global _golden
    if _golden is None:
        with np.load(PATH) as z:
            g = {k: z[k] for k in z.files}
        g["bone"] = from_bit_steps(g.pop("bone_bit_steps"))
        for a in g.values():
            a.setflags(write=False)
        _golden = g
    return _golden
