"""libscsfm_cast.so, the twenty-second library (scsfm_hip.libraries.FURTHER): the row stands in a seventh tuple and leaves
TABLE, LATER, NEWER, ROWS, NEWEST, EVERY, NEXT, ALL, BEYOND, LIBRARIES, SUMMARY and the keys of BY_NAME as they are, and
CATALOGUE covers every row; the header declares exactly the entry points; the library builds with hipcc for gfx950 (no GPU
needed), exports exactly them and carries the tree's source id; no other library's source id sees csrc_cast; bad arguments
are rejected with -1 (sizes with 0) before any pointer is touched; no kernel uses scratch or spills a register; build()
reports the library ahead of every other line, in a wording of its own, which leaves every older pin of the output in
place."""
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
ENTRY_POINTS = {"scsfm_cast_abi_version", "scsfm_cast_source_id", "scsfm_cast_views", "scsfm_cast_mask_bytes",
                "scsfm_cast_mask", "scsfm_cast_cast"}


def test_the_row_is_registered_in_a_seventh_tuple():
    assert [row.name for row in libraries.FURTHER] == ["cast"]
    assert [row.name for row in libraries.BEYOND] == ["mesh"] and [row.name for row in libraries.NEXT] == ["fuse"]
    assert [row.name for row in libraries.NEWEST] == ["pw"] and [row.name for row in libraries.NEWER] == ["opt"]
    assert [row.name for row in libraries.LATER] == ["fbn"] and len(libraries.TABLE) == 16
    assert set(libraries.BY_NAME) == {r.name for r in libraries.TABLE} | {"fbn"}
    assert libraries.ROWS == libraries.TABLE + libraries.LATER + libraries.NEWER
    assert libraries.EVERY == libraries.ROWS + libraries.NEWEST
    assert libraries.ALL == libraries.EVERY + libraries.NEXT and len(libraries.ALL) == 20
    assert libraries.LIBRARIES == libraries.ALL + libraries.BEYOND and len(libraries.LIBRARIES) == 21
    assert libraries.CATALOGUE == libraries.LIBRARIES + libraries.FURTHER and len(libraries.CATALOGUE) == 22
    assert len({r.name for r in libraries.CATALOGUE}) == 22
    row = libraries.find("cast")
    assert row is libraries.FURTHER[0] and row.abi == 1 and row.tag == "cast:build" and not row.tag.startswith("build")
    assert all(libraries.find(r.name) is r for r in libraries.CATALOGUE)
    assert row.csrc.endswith("csrc_cast") and row.header.endswith("scsfm_cast.h")
    assert row.lib.endswith("libscsfm_cast.so") and row.prefix == "scsfm_cast_"
    assert len(libraries.SUMMARY.splitlines()) == 21 and "libscsfm_cast.so" not in libraries.SUMMARY
    assert build.CAST_LIB == row.lib and build.CAST_CSRC == row.csrc and _lib.CAST_HEADER == row.header
    assert _lib.CAST_LIB_PATH == row.lib and _lib.CAST_ABI_VERSION == 1 and callable(_lib.get_cast)
    assert row.what in _lib.get_cast.__doc__
    assert callable(build.build_cast) and callable(build.cast_deps) and callable(build.cast_is_stale)
    assert [os.path.basename(p) for p in build.cast_sources()] == ["scsfm_cast.hip"]
    assert build.cast_source_id() == build.lib_source_id("cast")
    assert "libscsfm_cast.so" in libraries.__doc__ or "FURTHER" in libraries.__doc__


def test_other_source_ids_do_not_see_csrc_cast():
    ids = []
    for row in libraries.LIBRARIES:
        deps = build.lib_deps(row.name)
        assert deps and not any("csrc_cast" in p or "scsfm_cast" in p for p in deps), row.name
        ids.append(build.lib_source_id(row.name))
    assert all(os.sep + "csrc_cast" + os.sep in p or p.endswith("scsfm_cast.h") for p in build.cast_deps())
    assert len(set(ids)) == 21 and build.cast_source_id() not in ids


def test_header_declares_exactly_the_entry_points():
    decls = _lib.parse_header(_lib.CAST_HEADER)
    assert set(decls) == ENTRY_POINTS
    assert len(decls["scsfm_cast_views"][1]) == 5 and len(decls["scsfm_cast_mask"][1]) == 7
    assert len(decls["scsfm_cast_cast"][1]) == 22 and decls["scsfm_cast_mask_bytes"][0] is ctypes.c_size_t
    text = open(_lib.CAST_HEADER).read()
    for word in ("VALID", "INSIDE", "EVENT", "HIT", "ENDS WITHOUT A HIT", "0x7fc00000"):
        assert word in text, word


def _lib_cast():
    return _lib.CLib(build.build_cast(verbose=False), _lib.CAST_HEADER, _lib.CAST_ABI_VERSION, "scsfm_cast_")


@needs_hipcc
def test_cast_library_builds_and_exports_its_header():
    path = build.build_cast(verbose=False)
    assert path.endswith("libscsfm_cast.so")
    assert build.binary_source_id(path) == build.cast_source_id() and not build.cast_is_stale()
    lib = _lib_cast()
    assert lib.source_id() == build.cast_source_id()
    assert lib._fn["scsfm_cast_abi_version"]() == 1
    assert set(lib.decls) == ENTRY_POINTS
    nm = shutil.which("nm") or "/opt/rocm/llvm/bin/llvm-nm"
    syms = subprocess.run([nm, "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in syms.splitlines() if " T " in line and "scsfm" in line}
    assert exported == ENTRY_POINTS
    assert _lib.get_cast().path == path


@needs_hipcc
def test_argument_errors_return_minus_one():
    lib = _lib_cast()
    p = ctypes.c_void_p(4096)  # never dereferenced: every call below is rejected before anything is launched
    nan, inf, big = float("nan"), float("inf"), 2 ** 31 - 1
    mask_bytes = lib._fn["scsfm_cast_mask_bytes"]
    assert mask_bytes(40, 18, 29) == 5 * 3 * 4 and mask_bytes(1, 1, 1) == 1 and mask_bytes(8, 8, 9) == 2
    assert mask_bytes(1024, 1024, 512) == 2 ** 20 and mask_bytes(512, 128, 512) == 2 ** 16
    for dims in ((0, 4, 4), (4, -1, 4), (4, 4, 0), (1024, 1024, 513), (big, 1, 1), (big, big, big), (65536, 65536, 1),
                 (2 ** 29 + 1, 1, 1), (1, 2 ** 15, 2 ** 15)):
        assert mask_bytes(*dims) == 0, dims
    views, mask, cast = (lib._fn["scsfm_cast_" + k] for k in ("views", "mask", "cast"))
    odd2 = ctypes.c_void_p(4098)
    for args in ((0, p, p, p), (-3, p, p, p), (2 ** 27, p, p, p), (2, None, p, p), (2, p, None, p), (2, p, p, None)):
        assert views(*args, None) == -1, args
    #         nx ny nz volume min_weight mask
    good_m = [8, 6, 5, p, 1.0, p]
    for k, bad in ((0, 0), (2, -1), (0, 2 ** 30), (3, None), (3, odd2), (4, 0.5), (4, 0.0), (4, nan), (4, inf), (4, -inf),
                   (5, None)):
        args = list(good_m)
        args[k] = bad
        assert mask(*args, None) == -1, (k, bad)
    #         0  1  2  3    4    5    6     7      8          9    10   11      12 13 14 15   16   17    18     19  20
    #         nx ny nz ox   oy   oz   voxel volume min_weight near step n_steps V  H  W  view mask depth normal rgb shade
    good_c = [8, 6, 5, 0.0, 0.0, 0.0, 0.1, p, 1.0, 0.0, 0.1, 30, 2, 12, 20, p, p, p, p, p, p]
    for k, bad in ((0, 0), (1, -2), (2, 0), (0, 2 ** 29 + 1), (2, 2 ** 28), (3, nan), (4, inf), (5, -inf), (6, 0.0),
                   (6, -0.1), (6, nan), (6, inf), (7, None), (7, odd2), (8, 0.5), (8, nan), (8, inf), (9, -0.01), (9, nan),
                   (9, inf), (10, 0.0), (10, -0.1), (10, nan), (10, inf), (11, 0), (11, -1), (11, 2 ** 20 + 1), (12, 0),
                   (12, -1), (13, 0), (14, -4), (15, None), (15, odd2), (17, None), (17, odd2), (18, odd2), (13, 65536),
                   (12, big), (14, big)):
        args = list(good_c)
        args[k] = bad
        if k == 13 and bad == 65536:
            args[14] = 65536   # H W past int
        assert cast(*args, None) == -1, (k, bad)
    args = list(good_c)
    args[12], args[13], args[14] = 1024, 1024, 1024  # V 3 H W past int
    assert cast(*args, None) == -1
    assert lib._fn["scsfm_cast_source_id"](None, 64) == -1


@needs_hipcc
def test_no_kernel_spills_to_scratch(tmp_path):
    """The compiler's resource usage of the four kernels (read as tests/test_fuse_library.py reads it): no scratch and no
    spilled register."""
    out = tmp_path / "cast.s"
    flags = [f for f in build.FLAGS if f not in ("-shared", "-fPIC")]
    (src,) = build.cast_sources()
    subprocess.run([HIPCC, *flags, "-S", "--cuda-device-only", "-I", os.path.join(ROOT, "include"), "-o", str(out), src],
                   check=True, capture_output=True)
    text = open(out).read()
    kernels = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M)
    scratch = [int(x) for x in re.findall(r";\s*ScratchSize:\s*(\d+)", text)]
    spills = [int(x) for x in re.findall(r"\.[sv]gpr_spill_count:\s*(\d+)", text)]
    assert len(kernels) == 4 and len(scratch) == 4 and len(spills) == 8, (kernels, scratch, spills)
    assert sum("cast_kernel" in k for k in kernels) == 2
    assert sum("mask_kernel" in k for k in kernels) == 1 and sum("views_kernel" in k for k in kernels) == 1
    assert scratch == [0] * 4 and not any(spills), (scratch, spills)


@needs_hipcc
def test_build_reports_the_library_ahead_of_every_other_line(capsys):
    """The place the older pins leave: the line does not contain "entry points resolved" (twenty-one lines do, seventeen
    end in it), does not start with "[build" (ten do), stands ahead of opt's line, with which the window of seven pinned
    tags begins, and so ahead of vis and prep, which come last."""
    import sys
    sys.path.insert(0, ROOT)
    import __graft_entry__ as G
    G.build()
    out = capsys.readouterr().out.splitlines()
    mine = [i for i, line in enumerate(out) if line.startswith("[cast:build] ")]
    assert len(mine) == 1
    assert out[mine[0]] == f"[cast:build] {build.CAST_LIB}: ABI 1, {len(ENTRY_POINTS)} symbols of include/scsfm_cast.h"
    first = min(i for i, line in enumerate(out) if "entry points resolved" in line)
    assert mine[0] == first - 1 and out[first].startswith("[opt:build] ")
    tags = [line.split("]")[0] + "]" for line in out[first:first + 7]]
    assert tags == ["[opt:build]", "[pw:build]", "[fbn:build]", "[fuse:build]", "[dgrad:build]", "[mesh:build]",
                    "[vlog:build]"]
    assert len([line for line in out if line.endswith("entry points resolved")]) == 17
    assert len([line for line in out if "entry points resolved" in line]) == 21
    assert len([line for line in out if line.startswith("[build")]) == 10
    assert out[-2].startswith("[build:vis] ") and out[-1].startswith("[build:prep] ")
    import scsfm_hip.raycast  # noqa: F401  (build() imports it)
    assert "scsfm_hip.raycast" in sys.modules
