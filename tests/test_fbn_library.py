"""libscsfm_fbn.so, the seventeenth library (scsfm_hip.libraries.LATER): builds with hipcc for gfx950 (no GPU needed),
exports exactly the symbols include/scsfm_fbn.h declares, rejects bad arguments with -1 before touching any pointer --
the parameter gradients given by halves and a short workspace among them --, leaves the sixteen rows of the table and
their source ids alone, none of its kernels spills to scratch or needs more than 64 vector registers, and build() reports
it under its own tag ahead of every other line."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

from scsfm_hip import _lib, build, libraries

HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
needs_hipcc = pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc on this machine")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = {"scsfm_fbn_abi_version", "scsfm_fbn_source_id", "scsfm_fbn_workspace_bytes", "scsfm_fbn_bn_bwd_f32"}


def test_the_row_is_registered_beside_the_table():
    assert [row.name for row in libraries.LATER] == ["fbn"] and len(libraries.TABLE) == 16
    row = libraries.BY_NAME["fbn"]
    assert row is libraries.LATER[0] and row.abi == 1 and row.tag == "fbn:build" and not row.tag.startswith("build")
    assert row.csrc.endswith("csrc_fbn") and row.header.endswith("scsfm_fbn.h") and row.lib.endswith("libscsfm_fbn.so")
    assert row.prefix == "scsfm_fbn_" and set(libraries.BY_NAME) == {r.name for r in libraries.TABLE} | {"fbn"}
    assert "libscsfm_fbn.so" in libraries.SUMMARY and "libscsfm_fbn.so" in build.__doc__ and "libscsfm_fbn.so" in _lib.__doc__
    assert build.FBN_LIB == row.lib and build.FBN_CSRC == row.csrc and _lib.FBN_HEADER == row.header
    assert _lib.FBN_LIB_PATH == row.lib and _lib.FBN_ABI_VERSION == 1 and callable(_lib.get_fbn)
    assert os.path.basename(build.fbn_sources()[0]) == "scsfm_frozen_bn.hip" and len(build.fbn_sources()) == 1


def test_other_source_ids_do_not_see_csrc_fbn():
    ids = []
    for row in libraries.TABLE:
        deps = build.lib_deps(row.name)
        assert deps and not any("csrc_fbn" in p or "scsfm_fbn" in p for p in deps), row.name
        ids.append(build.lib_source_id(row.name))
    assert all(os.sep + "csrc_fbn" + os.sep in p or p.endswith("scsfm_fbn.h") for p in build.fbn_deps())
    assert len(set(ids)) == 16 and build.fbn_source_id() not in ids


def test_header_declares_exactly_the_entry_points():
    assert set(_lib.parse_header(_lib.FBN_HEADER)) == ENTRY_POINTS


def _lib_fbn():
    return _lib.CLib(build.build_fbn(verbose=False), _lib.FBN_HEADER, _lib.FBN_ABI_VERSION, "scsfm_fbn_")


@needs_hipcc
def test_fbn_library_builds_and_exports_its_header():
    path = build.build_fbn(verbose=False)
    assert path.endswith("libscsfm_fbn.so")
    assert build.binary_source_id(path) == build.fbn_source_id() and not build.fbn_is_stale()
    lib = _lib_fbn()
    assert lib.source_id() == build.fbn_source_id()
    assert lib._fn["scsfm_fbn_abi_version"]() == 1
    assert set(lib.decls) == ENTRY_POINTS
    nm = shutil.which("nm") or "/opt/rocm/llvm/bin/llvm-nm"
    syms = subprocess.run([nm, "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in syms.splitlines() if " T " in line and "scsfm" in line}
    assert exported == ENTRY_POINTS
    assert _lib.get_fbn().path == path


@needs_hipcc
def test_argument_errors_return_minus_one():
    lib = _lib_fbn()
    p = ctypes.c_void_p(256)  # never dereferenced: every call below is rejected before anything is launched
    nan, inf = float("nan"), float("inf")
    fn = lib._fn["scsfm_fbn_bn_bwd_f32"]
    need = lib.size("scsfm_fbn_workspace_bytes", 2, 4, 3, 5)
    assert need >= 2 * 4 * 16
    #       B  C  H  W  mode eps  g  x  y  gamma rm rv dx d_id dgamma dbeta ws ws_bytes stream
    good = [2, 4, 3, 5, 2, 1e-5, p, p, p, p, p, p, p, p, p, p, p, need, None]
    for k, bad in ((0, 0), (1, 0), (2, -1), (3, 0), (0, 1 << 30), (4, 3), (4, -1), (5, -1e-5), (5, nan), (5, inf),
                   (5, -inf), (6, None), (7, None), (8, None), (9, None), (10, None), (11, None), (12, None), (13, None),
                   (14, None), (15, None), (16, None), (16, ctypes.c_void_p(260)), (17, need - 1), (17, 0)):
        args = list(good)
        args[k] = bad
        assert fn(*args) == -1, (k, bad)
    assert fn(1 << 15, 1 << 8, 1 << 4, 1 << 4, 1, 1e-5, *[p] * 11, 1 << 40, None) == -1  # 2^31 elements
    # the parameter gradients by halves: each of dgamma / dbeta alone, with and without x and the workspace
    for dgamma, dbeta in ((p, None), (None, p)):
        for x in (p, None):
            for ws, n in ((p, need), (None, 0)):
                assert fn(2, 4, 3, 5, 1, 1e-5, p, x, p, p, p, p, p, None, dgamma, dbeta, ws, n, None) == -1
    # without the ReLU's output in modes 1 and 2, without d_identity in mode 2, in the no-parameter form too
    assert fn(2, 4, 3, 5, 1, 1e-5, p, None, None, p, None, p, p, None, None, None, None, 0, None) == -1
    assert fn(2, 4, 3, 5, 2, 1e-5, p, None, p, p, None, p, p, None, None, None, None, 0, None) == -1
    assert lib.size("scsfm_fbn_workspace_bytes", 0, 4, 3, 5) == 0
    assert lib.size("scsfm_fbn_workspace_bytes", 1 << 15, 1 << 8, 1 << 4, 1 << 4) == 0
    assert lib._fn["scsfm_fbn_source_id"](None, 64) == -1


@needs_hipcc
def test_no_kernel_spills_to_scratch(tmp_path):
    """The compiler's resource usage of every kernel of the library (read as tests/test_encoder_eval_library.py reads it):
    no scratch, no LDS, and at most 64 vector registers so that eight waves per SIMD stay resident -- these kernels hide
    memory latency with occupancy."""
    out = tmp_path / "fbn.s"
    flags = [f for f in build.FLAGS if f not in ("-shared", "-fPIC")]
    (src,) = build.fbn_sources()
    subprocess.run([HIPCC, *flags, "-S", "--cuda-device-only", "-I", os.path.join(ROOT, "include"), "-o", str(out), src],
                   check=True, capture_output=True)
    text = open(out).read()
    kernels = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M)
    scratch = [int(x) for x in re.findall(r";\s*ScratchSize:\s*(\d+)", text)]
    vgprs = [int(x) for x in re.findall(r";\s*NumVgprs:\s*(\d+)", text)]
    lds = [int(x) for x in re.findall(r";\s*LDSByteSize:\s*(\d+)", text)]
    # the backward: 2 widths x 3 modes x (with, without parameter gradients); the second launch that adds the slots
    assert len(kernels) == 13 and len(scratch) == len(kernels) == len(vgprs) == len(lds), (kernels, scratch)
    assert all(s == 0 for s in scratch), dict(zip(kernels, scratch))
    assert all(v <= 64 for v in vgprs), dict(zip(kernels, vgprs))
    assert all(b == 0 for b in lds), dict(zip(kernels, lds))


@needs_hipcc
def test_build_reports_the_library_ahead_of_every_other_line(capsys):
    import sys
    sys.path.insert(0, ROOT)
    import __graft_entry__ as G
    G.build()
    out = capsys.readouterr().out.splitlines()
    mine = [i for i, line in enumerate(out) if line.startswith("[fbn:build] ")]
    assert len(mine) == 1
    assert out[mine[0]] == f"[fbn:build] {build.FBN_LIB}: {len(ENTRY_POINTS)} entry points resolved"
    reports = [i for i, line in enumerate(out) if line.endswith("entry points resolved")]
    assert mine[0] == reports[0] and len(reports) == 17
    assert len([line for line in out if line.startswith("[build")]) == 10
