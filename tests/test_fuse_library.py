"""libscsfm_fuse.so, the twentieth library (scsfm_hip.libraries.NEXT): the row stands in a fifth tuple and leaves TABLE,
LATER, NEWER, ROWS, NEWEST, EVERY and the keys of BY_NAME as they are, and ALL covers every row; the header declares
exactly the entry points; the library builds with hipcc for gfx950 (no GPU needed), exports exactly them and carries the
tree's source id; no other library's source id sees csrc_fuse; bad arguments are rejected with -1 (sizes with 0) before any
pointer is touched; no kernel uses scratch or spills a register; build() reports the library directly behind fbn's line,
in opt's and pw's wording, which leaves every older pin of the output in place."""
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
ENTRY_POINTS = {"scsfm_fuse_abi_version", "scsfm_fuse_source_id", "scsfm_fuse_volume_bytes", "scsfm_fuse_cameras",
                "scsfm_fuse_integrate", "scsfm_fuse_extract_ws_bytes", "scsfm_fuse_count", "scsfm_fuse_extract"}


def test_the_row_is_registered_in_a_fifth_tuple():
    assert [row.name for row in libraries.NEXT] == ["fuse"]
    assert [row.name for row in libraries.NEWEST] == ["pw"] and [row.name for row in libraries.NEWER] == ["opt"]
    assert [row.name for row in libraries.LATER] == ["fbn"] and len(libraries.TABLE) == 16
    assert set(libraries.BY_NAME) == {r.name for r in libraries.TABLE} | {"fbn"}
    assert libraries.ROWS == libraries.TABLE + libraries.LATER + libraries.NEWER
    assert libraries.EVERY == libraries.ROWS + libraries.NEWEST
    assert libraries.ALL == libraries.EVERY + libraries.NEXT and len(libraries.ALL) == 20
    assert len({r.name for r in libraries.ALL}) == 20
    row = libraries.find("fuse")
    assert row is libraries.NEXT[0] and row.abi == 1 and row.tag == "fuse:build" and not row.tag.startswith("build")
    assert all(libraries.find(r.name) is r for r in libraries.ALL)
    assert row.csrc.endswith("csrc_fuse") and row.header.endswith("scsfm_fuse.h")
    assert row.lib.endswith("libscsfm_fuse.so") and row.prefix == "scsfm_fuse_"
    for text in (libraries.SUMMARY, build.__doc__, _lib.__doc__):
        assert "libscsfm_fuse.so" in text and "libscsfm_pw.so" in text
    assert build.FUSE_LIB == row.lib and build.FUSE_CSRC == row.csrc and _lib.FUSE_HEADER == row.header
    assert _lib.FUSE_LIB_PATH == row.lib and _lib.FUSE_ABI_VERSION == 1 and callable(_lib.get_fuse)
    assert row.what in _lib.get_fuse.__doc__
    assert callable(build.build_fuse) and callable(build.fuse_deps) and callable(build.fuse_is_stale)
    assert [os.path.basename(p) for p in build.fuse_sources()] == ["scsfm_fuse.hip"]
    assert build.fuse_source_id() == build.lib_source_id("fuse")


def test_other_source_ids_do_not_see_csrc_fuse():
    ids = []
    for row in libraries.EVERY:
        deps = build.lib_deps(row.name)
        assert deps and not any("csrc_fuse" in p or "scsfm_fuse" in p for p in deps), row.name
        ids.append(build.lib_source_id(row.name))
    assert all(os.sep + "csrc_fuse" + os.sep in p or p.endswith("scsfm_fuse.h") for p in build.fuse_deps())
    assert len(set(ids)) == 19 and build.fuse_source_id() not in ids


def test_header_declares_exactly_the_entry_points():
    decls = _lib.parse_header(_lib.FUSE_HEADER)
    assert set(decls) == ENTRY_POINTS
    assert len(decls["scsfm_fuse_integrate"][1]) == 20 and len(decls["scsfm_fuse_extract"][1]) == 15


def _lib_fuse():
    return _lib.CLib(build.build_fuse(verbose=False), _lib.FUSE_HEADER, _lib.FUSE_ABI_VERSION, "scsfm_fuse_")


@needs_hipcc
def test_fuse_library_builds_and_exports_its_header():
    path = build.build_fuse(verbose=False)
    assert path.endswith("libscsfm_fuse.so")
    assert build.binary_source_id(path) == build.fuse_source_id() and not build.fuse_is_stale()
    lib = _lib_fuse()
    assert lib.source_id() == build.fuse_source_id()
    assert lib._fn["scsfm_fuse_abi_version"]() == 1
    assert set(lib.decls) == ENTRY_POINTS
    nm = shutil.which("nm") or "/opt/rocm/llvm/bin/llvm-nm"
    syms = subprocess.run([nm, "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in syms.splitlines() if " T " in line and "scsfm" in line}
    assert exported == ENTRY_POINTS
    assert _lib.get_fuse().path == path


@needs_hipcc
def test_argument_errors_return_minus_one():
    lib = _lib_fuse()
    p = ctypes.c_void_p(4096)  # never dereferenced: every call below is rejected before anything is launched
    nan, inf, big = float("nan"), float("inf"), 2 ** 31 - 1
    vol_bytes, ws_bytes = lib._fn["scsfm_fuse_volume_bytes"], lib._fn["scsfm_fuse_extract_ws_bytes"]
    assert vol_bytes(37, 18, 29) == 20 * 37 * 18 * 29 and vol_bytes(1024, 1024, 512) == 20 * 2 ** 29
    assert ws_bytes(37, 18, 29) == 4 * (4 + 2 * 19) and ws_bytes(1024, 1024, 512) == 4 * (4 + 2 * 2 ** 19)
    for dims in ((0, 4, 4), (4, -1, 4), (4, 4, 0), (1024, 1024, 513), (big, 1, 1), (big, big, big), (65536, 65536, 1),
                 (2 ** 29 + 1, 1, 1), (1, 2 ** 15, 2 ** 15)):
        assert vol_bytes(*dims) == 0 and ws_bytes(*dims) == 0, dims
    assert vol_bytes(2 ** 29, 1, 1) == 20 * 2 ** 29
    cameras, integrate = lib._fn["scsfm_fuse_cameras"], lib._fn["scsfm_fuse_integrate"]
    count, extract = lib._fn["scsfm_fuse_count"], lib._fn["scsfm_fuse_extract"]
    for args in ((0, p, p, p), (-3, p, p, p), (2, None, p, p), (2, p, None, p), (2, p, p, None), (big, p, p, p)):
        assert cameras(*args, None) == -1, args
    #       0  1  2  3    4    5    6    7     8     9    10    11 12 13 14 15 16 17 18
    #       nx ny nz ox   oy   oz   vox  trunc near  maxd maxw  F  H  W cam depth disp image volume
    good = [8, 6, 5, 0.0, 0.0, 0.0, 0.1, 0.3, 0.05, 4.0, 64.0, 2, 12, 20, p, p, 1, p, p]
    for k, bad in ((0, 0), (1, -2), (2, 0), (0, 2 ** 29 + 1), (2, 2 ** 28), (3, nan), (4, inf), (5, -inf), (6, 0.0),
                   (6, -0.1), (6, nan), (6, inf), (7, 0.0), (7, -1.0), (7, nan), (8, -0.01), (8, nan), (9, 0.0), (9, nan),
                   (10, 0.5), (10, nan), (10, inf), (11, 0), (11, -1), (12, 0), (13, -4), (14, None), (15, None),
                   (18, None), (18, ctypes.c_void_p(4098)), (12, 65536), (11, big), (13, big)):
        args = list(good)
        args[k] = bad
        if k == 12 and bad == 65536:
            args[13] = 65536   # H W past int
        assert integrate(*args, None) == -1, (k, bad)
    args = list(good)
    args[11], args[12], args[13] = 1024, 1024, 1024  # F 3 H W past int
    assert integrate(*args, None) == -1
    n = ws_bytes(8, 6, 5)
    #         nx ny nz volume min_weight ws ws_bytes
    good_c = [8, 6, 5, p, 1.0, p, n]
    for k, bad in ((0, 0), (2, -1), (0, 2 ** 30), (3, None), (4, 0.5), (4, 0.0), (4, nan), (4, inf), (5, None),
                   (5, ctypes.c_void_p(4100)), (6, n - 4), (6, 0)):
        args = list(good_c)
        args[k] = bad
        assert count(*args, None) == -1, (k, bad)
    #         nx ny nz ox   oy   oz   voxel volume min_weight ws ws_bytes capacity xyz rgb
    good_e = [8, 6, 5, 0.0, 0.0, 0.0, 0.1, p, 1.0, p, n, 10, p, p]
    for k, bad in ((0, 0), (1, 2 ** 30), (3, nan), (6, 0.0), (6, nan), (7, None), (8, 0.99), (8, nan), (9, None),
                   (9, ctypes.c_void_p(4104)), (10, n - 1), (11, -1), (12, None), (13, None)):
        args = list(good_e)
        args[k] = bad
        assert extract(*args, None) == -1, (k, bad)
    assert lib._fn["scsfm_fuse_source_id"](None, 64) == -1


@needs_hipcc
def test_no_kernel_spills_to_scratch(tmp_path):
    """The compiler's resource usage of the eight kernels (read as tests/test_pw_library.py reads it): no scratch and no
    spilled register."""
    out = tmp_path / "fuse.s"
    flags = [f for f in build.FLAGS if f not in ("-shared", "-fPIC")]
    (src,) = build.fuse_sources()
    subprocess.run([HIPCC, *flags, "-S", "--cuda-device-only", "-I", os.path.join(ROOT, "include"), "-o", str(out), src],
                   check=True, capture_output=True)
    text = open(out).read()
    kernels = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M)
    scratch = [int(x) for x in re.findall(r";\s*ScratchSize:\s*(\d+)", text)]
    spills = [int(x) for x in re.findall(r"\.[sv]gpr_spill_count:\s*(\d+)", text)]
    assert len(kernels) == 8 and len(scratch) == 8 and len(spills) == 16, (kernels, scratch, spills)
    for name in ("cameras_kernel", "integrate_kernel", "extract_kernel", "scan_kernel"):
        assert any(name in k for k in kernels), name
    assert scratch == [0] * 8 and not any(spills), (scratch, spills)


@needs_hipcc
def test_build_reports_the_library_directly_behind_the_later_lines(capsys):
    """The one place and wording the older pins leave: opt's line is the first with "entry points resolved", pw's the
    next and fbn's directly behind it; seventeen lines END in the phrase, so this one does not (it carries "(ABI 1)", as
    opt's and pw's); ten start with "[build", vis and prep come last."""
    import sys
    sys.path.insert(0, ROOT)
    import __graft_entry__ as G
    G.build()
    out = capsys.readouterr().out.splitlines()
    mine = [i for i, line in enumerate(out) if line.startswith("[fuse:build] ")]
    assert len(mine) == 1
    assert out[mine[0]] == f"[fuse:build] {build.FUSE_LIB}: {len(ENTRY_POINTS)} entry points resolved (ABI 1)"
    first = min(i for i, line in enumerate(out) if "entry points resolved" in line)
    assert out[first].startswith("[opt:build] ") and out[first + 1].startswith("[pw:build] ")
    assert out[first + 2].startswith("[fbn:build] ") and mine[0] == first + 3
    reports = [i for i, line in enumerate(out) if line.endswith("entry points resolved")]
    assert len(reports) == 17 and reports[0] == first + 2 and reports[1] == mine[0] + 1
    assert len([line for line in out if line.startswith("[build")]) == 10
    assert out[-2].startswith("[build:vis] ") and out[-1].startswith("[build:prep] ")
