"""Compile one library of scsfm_hip/libraries.py's table (every row but the loss library, which tests/hostsim/build.py
builds per object), unchanged, against tests/hostsim/hip/hip_runtime.h with g++ into
tests/hostsim/_build_<name>/libscsfm_<name>_hostsim.so: the same C ABI with HOST pointers.  tests/_hostsim_<name>.py
calls it and wraps the entry points.  Test infrastructure only; never loaded by the product."""
from __future__ import annotations

import glob
import os
import subprocess

from scsfm_hip.libraries import BY_NAME

HERE = os.path.dirname(os.path.abspath(__file__))


def build(name, force=False, src=None, lib=None, shim=None, dep=None):
    """-> the simulator's library of row ``name``, compiled when it is missing or older than a source, a header, the
    ``shim`` (injected with -include) or ``dep`` (the calling tests/_hostsim_<name>.py).  ``src`` and ``lib`` stand in
    for the row's source directory and for the output (tests that compile an edited copy)."""
    row = BY_NAME[name]
    src = src or row.csrc
    lib = lib or os.path.join(HERE, f"_build_{name}", f"libscsfm_{name}_hostsim.so")
    inject = ["-include", shim] if shim else []
    srcs = sorted(glob.glob(os.path.join(src, "*.hip")))
    deps = srcs + glob.glob(os.path.join(src, "*.h")) + [os.path.join(HERE, "hip", "hip_runtime.h"), row.header] + \
        [d for d in (shim, dep) if d]
    if not force and os.path.exists(lib) and all(os.path.getmtime(d) <= os.path.getmtime(lib) for d in deps):
        return lib
    os.makedirs(os.path.dirname(lib), exist_ok=True)
    tmp = f"{lib}.{os.getpid()}.tmp"
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-x", "c++", "-I", HERE,
                    "-I", os.path.dirname(row.header), *inject, "-Wall", "-Wno-unused-function",
                    "-Wno-unknown-pragmas", "-o", tmp, *srcs], check=True)
    os.replace(tmp, lib)
    return lib
