"""libscsfm_val.so at ABI 2: the library still builds with hipcc for gfx950 (no GPU needed) from both files of csrc_val/,
exports exactly the header's symbols -- the three calls of the validation table among them -- carries the tree's source
id, rejects bad arguments of the new calls with -1 before anything is launched, and none of its kernels, the three new
ones included, spills to scratch; the table of libraries still has its sixteen rows."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

from scsfm_hip import _lib, build
from scsfm_hip.libraries import BY_NAME, TABLE

HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
needs_hipcc = pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc on this machine")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"scsfm_val_depth_errors_row", "scsfm_val_losses_row", "scsfm_val_table_mean"}
ENTRY_POINTS = NEW | {"scsfm_val_abi_version", "scsfm_val_source_id", "scsfm_val_workspace_bytes", "scsfm_val_depth_errors"}


def test_the_row_is_at_abi_2_and_no_row_was_added():
    assert len(TABLE) == 16 and BY_NAME["val"].abi == _lib.VAL_ABI_VERSION == 2
    assert "--with-gt" in BY_NAME["val"].what and "--shard-validation" in BY_NAME["val"].what
    assert [os.path.basename(p) for p in build.val_sources()] == ["scsfm_validation.hip", "scsfm_validation_table.hip"]
    assert set(_lib.parse_header(_lib.VAL_HEADER)) == ENTRY_POINTS
    assert "ABI 2" in open(_lib.VAL_HEADER).read()


@needs_hipcc
def test_val_library_builds_and_exports_its_header():
    path = build.build_val(verbose=False)
    assert build.binary_source_id(path) == build.val_source_id() and not build.val_is_stale()
    lib = _lib.CLib(path, _lib.VAL_HEADER, _lib.VAL_ABI_VERSION, "scsfm_val_")
    assert lib.source_id() == build.val_source_id() and lib._fn["scsfm_val_abi_version"]() == 2
    nm = shutil.which("nm") or "/opt/rocm/llvm/bin/llvm-nm"
    syms = subprocess.run([nm, "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in syms.splitlines() if " T " in line and "scsfm" in line}
    assert exported == ENTRY_POINTS

    p = ctypes.c_void_p(256)  # never dereferenced: every call below is rejected before anything is launched
    fn = lib._fn["scsfm_val_losses_row"]
    for k in range(4):
        args = [p, p, p, p]
        args[k] = None
        assert fn(*args, None) == -1, k
    fn = lib._fn["scsfm_val_table_mean"]
    for n_rows, table, out in ((0, p, p), (-2, p, p), (1 << 28, p, p), (4, None, p), (4, p, None)):
        assert fn(n_rows, table, out, None) == -1, (n_rows, table, out)
    fn = lib._fn["scsfm_val_depth_errors_row"]
    #       B  h  w   src is_disp H   W   gt y1 y2  x1 x2   min  max   lo    ws bytes    metrics medians count row stream
    good = [2, 8, 26, p, 1, 16, 52, p, 6, 15, 1, 50, 0.1, 80.0, 1e-3, p, 1 << 20, p, p, p, p, None]
    for k, bad in ((20, None), (0, 0), (1, 0), (5, -1), (8, 20), (12, 90.0), (16, 16), (3, None), (7, None), (15, None),
                   (17, None), (18, None), (19, None)):
        args = list(good)
        args[k] = bad
        assert fn(*args) == -1, (k, bad)


@needs_hipcc
def test_no_kernel_of_the_library_spills(tmp_path):
    """The compiler's resource usage of every kernel, read as tests/test_vlog_library.py reads it."""
    flags = [f for f in build.FLAGS if f not in ("-shared", "-fPIC")]
    found = {}
    for src in build.val_sources():
        out = tmp_path / (os.path.basename(src) + ".s")
        subprocess.run([HIPCC, *flags, "-S", "--cuda-device-only", "-I", os.path.join(ROOT, "include"), "-o", str(out),
                        src], check=True, capture_output=True)
        text = open(out).read()
        kernels = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M)
        scratch = [int(x) for x in re.findall(r";\s*ScratchSize:\s*(\d+)", text)]
        assert len(scratch) == len(kernels), (kernels, scratch)
        assert all(s == 0 for s in scratch), dict(zip(kernels, scratch))
        found[os.path.basename(src)] = kernels
    assert len(found["scsfm_validation.hip"]) == 4  # count, scan, compact, select
    table = found["scsfm_validation_table.hip"]
    assert len(table) == 3 and all(any(n in k for k in table) for n in ("batch_row", "losses_row", "table_mean"))
