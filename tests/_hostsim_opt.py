"""Compiles the one-launch Adam (sc-sfmlearner-release_amd/csrc_opt/*.hip), unchanged, against the host simulator
(tests/hostsim/hip/hip_runtime.h) into tests/hostsim/_build_opt/ and loads the C ABI of include/scsfm_opt.h on HOST
pointers.  The row is not one of scsfm_hip.libraries.BY_NAME's, which tests/hostsim/library.py looks its rows up in, so
this module has the g++ line itself: library.py's flags.  Test infrastructure only; never loaded by the product."""
from __future__ import annotations

import functools
import glob
import os
import subprocess

from scsfm_hip import libraries
from scsfm_hip._lib import OPT_ABI_VERSION, OPT_HEADER, CLib

HERE = os.path.dirname(os.path.abspath(__file__))
HOSTSIM = os.path.join(HERE, "hostsim")
LIB = os.path.join(HOSTSIM, "_build_opt", "libscsfm_opt_hostsim.so")


def build(force=False):
    row = libraries.find("opt")
    srcs = sorted(glob.glob(os.path.join(row.csrc, "*.hip")))
    deps = srcs + [os.path.join(HOSTSIM, "hip", "hip_runtime.h"), row.header, os.path.abspath(__file__)]
    if not force and os.path.exists(LIB) and all(os.path.getmtime(d) <= os.path.getmtime(LIB) for d in deps):
        return LIB
    os.makedirs(os.path.dirname(LIB), exist_ok=True)
    tmp = f"{LIB}.{os.getpid()}.tmp"
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-x", "c++", "-I", HOSTSIM,
                    "-I", os.path.dirname(row.header), "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas", "-o", tmp,
                    *srcs], check=True)
    os.replace(tmp, LIB)
    return LIB


@functools.lru_cache(maxsize=1)
def lib():
    return CLib(build(), OPT_HEADER, OPT_ABI_VERSION, "scsfm_opt_")
