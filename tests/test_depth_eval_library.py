"""libscsfm_eval.so: builds with hipcc for gfx950 (no GPU needed), exports exactly the symbols include/scsfm_eval.h
declares, rejects bad arguments with -1 before touching any pointer, and leaves the other two libraries' source ids
alone (the loss library's id ties the recorded PMC counters under profiles/ to its sources)."""
import ctypes
import os
import shutil
import subprocess

import pytest

from scsfm_hip import _lib, build

LOSS_ID = "a4885409350e4bef"  # (since the speculation weights are rounded to the element type; dc1122dba412f24a before)
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
needs_hipcc = pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc on this machine")


def test_other_source_ids_do_not_see_csrc_eval():
    assert build.source_id() == LOSS_ID
    assert not any("csrc_eval" in p or "scsfm_eval" in p for p in build.deps() + build.nets_deps())
    assert build.eval_sources() and all("csrc_eval" in p for p in build.eval_sources())
    assert build.eval_source_id() not in (build.source_id(), build.nets_source_id())


@needs_hipcc
def test_eval_library_builds_and_exports_its_header():
    path = build.build_eval(verbose=False)
    assert build.binary_source_id(path) == build.eval_source_id()
    lib = _lib.CLib(path, _lib.EVAL_HEADER, _lib.EVAL_ABI_VERSION, "scsfm_eval_")
    assert lib.source_id() == build.eval_source_id()
    assert set(lib.decls) == {"scsfm_eval_abi_version", "scsfm_eval_source_id", "scsfm_eval_workspace_bytes",
                              "scsfm_eval_depth"}
    nm = shutil.which("nm") or "/opt/rocm/llvm/bin/llvm-nm"
    syms = subprocess.run([nm, "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in syms.splitlines() if " T " in line and "scsfm" in line}
    assert exported == set(lib.decls)


@needs_hipcc
def test_argument_errors_return_minus_one():
    lib = _lib.CLib(build.build_eval(verbose=False), _lib.EVAL_HEADER, _lib.EVAL_ABI_VERSION, "scsfm_eval_")
    fn = lib._fn["scsfm_eval_depth"]
    p = ctypes.c_void_p(256)  # never dereferenced: every call below is rejected before anything is launched
    nbytes = lib.size("scsfm_eval_workspace_bytes", 2, 100, 200, 1, 0)
    assert nbytes >= 200 * 12
    assert lib.size("scsfm_eval_workspace_bytes", 0, 100, 200, 1, 0) == 0
    assert lib.size("scsfm_eval_workspace_bytes", 2, 0, 200, 1, 0) == 0
    good = [2, 8, 8, 1, p, 0, p, p, p, p, 100, 200, 1, 1e-3, 80.0, p, nbytes, p, p, p, p, None]
    for k, bad in ((0, 0), (1, 0), (2, -1), (4, None), (6, None), (7, None), (8, None), (9, None), (10, 0), (11, 0),
                   (13, 80.0), (15, None), (16, nbytes - 1), (17, None), (18, None), (19, None), (20, None)):
        args = list(good)
        args[k] = bad
        assert fn(*args) == -1, (k, bad)
