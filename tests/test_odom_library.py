"""libscsfm_odom.so: builds with hipcc for gfx950 (no GPU needed), exports exactly the symbols include/scsfm_odom.h
declares, rejects bad arguments with -1 before touching any pointer, leaves the other three libraries' source ids alone,
and none of its kernels spills to scratch."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

from scsfm_hip import _lib, build

LOSS_ID = "a4885409350e4bef"  # (since the speculation weights are rounded to the element type; dc1122dba412f24a before)
NETS_ID = "5e9e8a56c343fa9b"
EVAL_ID = "fcc94374d9bcd5ba"
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
needs_hipcc = pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc on this machine")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_other_source_ids_do_not_see_csrc_odom():
    assert (build.source_id(), build.nets_source_id(), build.eval_source_id()) == (LOSS_ID, NETS_ID, EVAL_ID)
    assert not any("csrc_odom" in p or "scsfm_odom" in p for p in build.deps() + build.nets_deps() + build.eval_deps())
    assert build.odom_sources() and all("csrc_odom" in p for p in build.odom_sources())
    assert build.odom_source_id() not in (LOSS_ID, NETS_ID, EVAL_ID)


def _lib_odom():
    return _lib.CLib(build.build_odom(verbose=False), _lib.ODOM_HEADER, _lib.ODOM_ABI_VERSION, "scsfm_odom_")


@needs_hipcc
def test_odom_library_builds_and_exports_its_header():
    path = build.build_odom(verbose=False)
    assert build.binary_source_id(path) == build.odom_source_id() and not build.odom_is_stale()
    lib = _lib_odom()
    assert lib.source_id() == build.odom_source_id()
    assert set(lib.decls) == {"scsfm_odom_abi_version", "scsfm_odom_source_id", "scsfm_odom_chain_workspace_bytes",
                              "scsfm_odom_chain", "scsfm_odom_eval_max_segments", "scsfm_odom_eval_workspace_bytes",
                              "scsfm_odom_eval"}
    nm = shutil.which("nm") or "/opt/rocm/llvm/bin/llvm-nm"
    syms = subprocess.run([nm, "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in syms.splitlines() if " T " in line and "scsfm" in line}
    assert exported == set(lib.decls)
    assert _lib.get_odom().path == path


@needs_hipcc
def test_argument_errors_return_minus_one():
    lib = _lib_odom()
    p = ctypes.c_void_p(256)  # never dereferenced: every call below is rejected before anything is launched
    assert lib.size("scsfm_odom_chain_workspace_bytes", 2, 1000) >= 2 * 4 * 96 * 2
    assert lib.size("scsfm_odom_chain_workspace_bytes", 0, 1000) == 0
    assert lib.size("scsfm_odom_chain_workspace_bytes", 2, -1) == 0
    nbytes = lib.size("scsfm_odom_chain_workspace_bytes", 2, 1000)
    fn = lib._fn["scsfm_odom_chain"]
    good = [2, 1000, 0, 0, p, p, p, p, None, p, p, nbytes, None]
    for k, bad in ((0, 0), (1, -1), (3, 2), (4, None), (5, None), (6, None), (7, None), (9, None), (10, None),
                   (11, nbytes - 1)):
        args = list(good)
        args[k] = bad
        assert fn(*args) == -1, (k, bad)

    assert lib.size("scsfm_odom_eval_max_segments", 1591) == 8 * 160
    assert lib.size("scsfm_odom_eval_max_segments", 0) == 0
    assert lib.size("scsfm_odom_eval_workspace_bytes", 2, 0, 10) == 0
    assert lib.size("scsfm_odom_eval_workspace_bytes", 2, 10, 0) == 0
    nbytes = lib.size("scsfm_odom_eval_workspace_bytes", 2, 1591, 2000)
    assert nbytes >= 2000 * (96 + 4 * 8) + 2 * 1280 * 40
    fn = lib._fn["scsfm_odom_eval"]
    good = [2, 1591, 2000, 3, p, p, p, p, 1280, p, nbytes, p, p, p, p, p, p, None]
    for k, bad in ((0, 0), (1, 0), (2, 0), (3, 5), (3, -1), (4, None), (5, None), (6, None), (7, None), (8, 1279),
                   (9, None), (10, nbytes - 1), (11, None), (12, None), (13, None), (14, None), (15, None), (16, None)):
        args = list(good)
        args[k] = bad
        assert fn(*args) == -1, (k, bad)


@needs_hipcc
def test_no_kernel_spills_to_scratch(tmp_path):
    """The compiler's resource usage of every kernel of the library (read as tests/test_kernel_resources.py reads it):
    no scratch, and at most 128 vector registers so that four waves per SIMD stay resident."""
    out = tmp_path / "odom.s"
    flags = [f for f in build.FLAGS if f not in ("-shared", "-fPIC")]
    for src in build.odom_sources():
        subprocess.run([HIPCC, *flags, "-S", "--cuda-device-only", "-I", os.path.join(ROOT, "include"), "-o", str(out),
                        src], check=True, capture_output=True)
        text = open(out).read()
        kernels = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M)
        scratch = [int(x) for x in re.findall(r";\s*ScratchSize:\s*(\d+)", text)]
        vgprs = [int(x) for x in re.findall(r";\s*NumVgprs:\s*(\d+)", text)]
        assert len(kernels) >= 9 and len(scratch) == len(kernels) == len(vgprs), (kernels, scratch)
        assert all(s == 0 for s in scratch), dict(zip(kernels, scratch))
        assert all(v <= 128 for v in vgprs), dict(zip(kernels, vgprs))
