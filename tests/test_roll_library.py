"""libscsfm_roll.so, the twenty-fifth library (scsfm_hip.libraries.ADDED): the row stands in the open-ended tuple and
REGISTRY covers it; the header declares exactly the entry points; the library builds with hipcc for gfx950 (no GPU needed),
exports exactly them and carries the tree's source id; no other library's source id sees csrc_roll, and csrc_roll includes
nothing of another library; bad arguments are rejected with -1 before any pointer is touched; no kernel uses scratch or
spills a register, and the shift moves 16 bytes per access; build() reports the library behind conf's line, in its
wording."""
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
ENTRY_POINTS = {"scsfm_roll_abi_version", "scsfm_roll_source_id", "scsfm_roll_shift", "scsfm_roll_ws_bytes",
                "scsfm_roll_count", "scsfm_roll_extract"}


def test_the_row_is_registered_in_the_open_ended_tuple():
    row = libraries.find("roll")
    assert row in libraries.ADDED and row in libraries.REGISTRY and row not in libraries.CATALOGUE
    assert libraries.REGISTRY == libraries.CATALOGUE + libraries.ADDED
    assert [r.name for r in libraries.ADDED[:3]] == ["track", "conf", "roll"]
    assert len({r.name for r in libraries.REGISTRY}) == len(libraries.REGISTRY) >= 25
    assert row.abi == 1 and row.tag == "roll:build" and not row.tag.startswith("build")
    assert row.csrc.endswith("csrc_roll") and row.header.endswith("scsfm_roll.h")
    assert row.lib.endswith("libscsfm_roll.so") and row.prefix == "scsfm_roll_"
    assert "libscsfm_roll.so" not in libraries.SUMMARY and "roll" not in libraries.BY_NAME
    for text in (libraries.SINCE, build.__doc__, _lib.__doc__):     # (the rows since SUMMARY was fixed are listed behind it)
        assert "libscsfm_roll.so" in text and "libscsfm_conf.so" in text and "include/scsfm_roll.h" in text
    assert build.ROLL_LIB == row.lib and build.ROLL_CSRC == row.csrc and _lib.ROLL_HEADER == row.header
    assert _lib.ROLL_LIB_PATH == row.lib and _lib.ROLL_ABI_VERSION == 1 and callable(_lib.get_roll)
    assert row.what in _lib.get_roll.__doc__
    assert callable(build.build_roll) and callable(build.roll_deps) and callable(build.roll_is_stale)
    assert [os.path.basename(p) for p in build.roll_sources()] == ["scsfm_roll.hip"]
    assert build.roll_source_id() == build.lib_source_id("roll")


def test_source_ids_are_per_library():
    ids = []
    for row in libraries.REGISTRY:
        if row.name == "roll":
            continue
        deps = build.lib_deps(row.name)
        assert deps and not any("csrc_roll" in p or "scsfm_roll" in p for p in deps), row.name
        ids.append(build.lib_source_id(row.name))
    assert all(os.sep + "csrc_roll" + os.sep in p or p.endswith("scsfm_roll.h") for p in build.roll_deps())
    assert len(set(ids)) == len(ids) and build.roll_source_id() not in ids
    # the extraction is restated, not shared: the source includes its own header and no other of the project's
    (src,) = build.roll_sources()
    mine = re.findall(r'#include\s+"([^"]+)"', open(src).read())
    assert mine == ["scsfm_roll.h"]
    assert not re.findall(r'#include\s+"', open(_lib.ROLL_HEADER).read())


def test_header_declares_exactly_the_entry_points():
    decls = _lib.parse_header(_lib.ROLL_HEADER)
    assert set(decls) == ENTRY_POINTS
    i, f, p, z = ctypes.c_int, ctypes.c_float, ctypes.c_void_p, ctypes.c_size_t
    assert decls["scsfm_roll_shift"] == (i, [i, i, i, i, i, i, p, p, p])
    assert decls["scsfm_roll_ws_bytes"] == (z, [i, i, i])
    # scsfm_fuse_count's and scsfm_fuse_extract's arguments with the six ints of the keep box in front of the volume
    fuse = _lib.parse_header(_lib.FUSE_HEADER)
    assert decls["scsfm_roll_ws_bytes"] == fuse["scsfm_fuse_extract_ws_bytes"]
    count, extract = fuse["scsfm_fuse_count"][1], fuse["scsfm_fuse_extract"][1]
    assert decls["scsfm_roll_count"] == (i, count[:3] + [i] * 6 + count[3:])
    assert decls["scsfm_roll_extract"] == (i, extract[:7] + [i] * 6 + extract[7:])
    text = open(_lib.ROLL_HEADER).read()
    for word in ("SCSFM_ROLL_CHUNK 1024", "o_k = fl(origin0 + fl(float(k) s))", "never accumulated",
                 "fl(o_k + fl(fl(float(i) + 0.5f) s))", "takes the BITS of src voxel (x + sx, y + sy, z + sz)",
                 "ONLY IF voxel a or voxel b lies outside the keep box", "x0 >= x1 or y0 >= y1 or z0 >= z1",
                 "does not load the volume", "[max(0, s), min(n, n + s))", "emitted at most once", "size_t"):
        assert word in text, word


def _lib_roll():
    return _lib.CLib(build.build_roll(verbose=False), _lib.ROLL_HEADER, _lib.ROLL_ABI_VERSION, "scsfm_roll_")


@needs_hipcc
def test_roll_library_builds_and_exports_its_header():
    path = build.build_roll(verbose=False)
    assert path.endswith("libscsfm_roll.so")
    assert build.binary_source_id(path) == build.roll_source_id() and not build.roll_is_stale()
    lib = _lib_roll()
    assert lib.source_id() == build.roll_source_id()
    assert lib._fn["scsfm_roll_abi_version"]() == 1
    assert set(lib.decls) == ENTRY_POINTS
    nm = shutil.which("nm") or "/opt/rocm/llvm/bin/llvm-nm"
    syms = subprocess.run([nm, "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in syms.splitlines() if " T " in line and "scsfm" in line}
    assert exported == ENTRY_POINTS
    assert _lib.get_roll().path == path


@needs_hipcc
def test_argument_errors_return_minus_one():
    lib = _lib_roll()
    p, q = ctypes.c_void_p(4096), ctypes.c_void_p(1 << 40)   # never dereferenced: every call below is rejected first
    odd2 = ctypes.c_void_p(4098)
    nan, inf = float("nan"), float("inf")
    shift, count, extract = (lib._fn["scsfm_roll_" + k] for k in ("shift", "count", "extract"))
    #            nx  ny  nz  sx sy sz src dst
    for args in ((0, 18, 29, 0, 0, 0, p, q), (37, -1, 29, 0, 0, 0, p, q), (37, 18, 0, 0, 0, 0, p, q),
                 (1024, 1024, 513, 0, 0, 0, p, q), (65536, 65536, 1, 0, 0, 0, p, q), (37, 18, 29, 1, 2, 3, None, q),
                 (37, 18, 29, 1, 2, 3, p, None), (37, 18, 29, 1, 2, 3, odd2, q), (37, 18, 29, 1, 2, 3, q, odd2),
                 (37, 18, 29, 1, 2, 3, p, p), (37, 18, 29, 0, 0, 0, p, ctypes.c_void_p(4096 + 4 * 5 * 19314 - 4)),
                 (37, 18, 29, 0, 0, 0, ctypes.c_void_p(4096 + 4 * 19314), p)):
        assert shift(*args, None) == -1, args
    n = lib.size("scsfm_roll_ws_bytes", 37, 18, 29)
    assert n == 4 * (4 + 2 * 19) and lib.size("scsfm_roll_ws_bytes", 0, 18, 29) == 0
    assert lib.size("scsfm_roll_ws_bytes", 1024, 1024, 513) == 0 and lib.size("scsfm_roll_ws_bytes", 1024, 1024, 512) > 0
    #       0   1   2   3 .. 8            9       10          11  12
    #       nx  ny  nz  the keep box      volume  min_weight  ws  ws_bytes
    good = [37, 18, 29, 0, 37, 0, 18, 8, 29, p, 1.0, p, n]
    for k, bad in ((0, 0), (1, -1), (2, 0), (9, None), (9, odd2), (10, 0.5), (10, nan), (10, inf), (11, None), (11, odd2),
                   (11, ctypes.c_void_p(4104)), (12, n - 4), (12, 0)):
        args = list(good)
        args[k] = bad
        assert count(*args, None) == -1, (k, bad)
    #       0   1   2   3    4    5    6      7 .. 12            13      14          15  16        17        18   19
    #       nx  ny  nz  ox   oy   oz   voxel  the keep box       volume  min_weight  ws  ws_bytes  capacity  xyz  rgb
    good = [37, 18, 29, 0.0, 0.0, 0.0, 0.1, 0, 37, 0, 18, 8, 29, p, 1.0, p, n, 7, p, p]
    for k, bad in ((0, 0), (1, -1), (2, 0), (3, nan), (4, inf), (5, -inf), (6, 0.0), (6, -0.1), (6, nan), (6, inf), (13, None),
                   (13, odd2), (14, 0.5), (14, nan), (15, None), (15, odd2), (16, n - 4), (17, -1), (18, None), (19, None)):
        args = list(good)
        args[k] = bad
        assert extract(*args, None) == -1, (k, bad)
    args = list(good)
    args[0], args[1], args[2] = 1024, 1024, 1024   # more than 2^29 voxels
    assert extract(*args, None) == -1 and count(*args[:3], *args[7:17], None) == -1
    assert lib._fn["scsfm_roll_source_id"](None, 64) == -1


@needs_hipcc
def test_no_kernel_spills_and_the_shift_moves_sixteen_bytes(tmp_path):
    """The compiler's resource usage of the four kernels (read as tests/test_conf_library.py reads it): no scratch and no
    spilled register.  The shift's kept path is one dwordx4 load and one dwordx4 store, its empty path one dwordx4 store."""
    out = tmp_path / "roll.s"
    flags = [f for f in build.FLAGS if f not in ("-shared", "-fPIC")]
    (src,) = build.roll_sources()
    subprocess.run([HIPCC, *flags, "-S", "--cuda-device-only", "-I", os.path.join(ROOT, "include"), "-o", str(out), src],
                   check=True, capture_output=True)
    text = open(out).read()
    kernels = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M)
    scratch = [int(x) for x in re.findall(r";\s*ScratchSize:\s*(\d+)", text)]
    spills = [int(x) for x in re.findall(r"\.[sv]gpr_spill_count:\s*(\d+)", text)]
    assert len(kernels) == 4 and len(scratch) == 4 and len(spills) == 8, (kernels, scratch, spills)
    for name, copies in (("shift_kernel", 1), ("extract_kernel", 2), ("scan_kernel", 1)):
        assert sum(name in k for k in kernels) == copies, name
    assert scratch == [0] * 4 and not any(spills), (scratch, spills)
    (name,) = [k for k in kernels if "shift_kernel" in k]
    body = text[text.index(name + ":"):]
    body = body[:body.index(".amdhsa_kernel")]
    assert len(re.findall(r"global_load_dwordx4", body)) == 1 and len(re.findall(r"global_store_dwordx4", body)) == 2, body


@needs_hipcc
def test_build_reports_the_library_behind_confs_line(capsys):
    """The line is in cast's wording: it does not contain "entry points resolved", does not start with "[build", and
    stands directly behind conf's line and ahead of cast's, which stays directly in front of opt's."""
    import sys
    sys.path.insert(0, ROOT)
    import __graft_entry__ as G
    G.build()
    out = capsys.readouterr().out.splitlines()
    mine = [i for i, line in enumerate(out) if line.startswith("[roll:build] ")]
    assert len(mine) == 1
    assert out[mine[0]] == f"[roll:build] {build.ROLL_LIB}: ABI 1, {len(ENTRY_POINTS)} symbols of include/scsfm_roll.h"
    cast = [i for i, line in enumerate(out) if line.startswith("[cast:build] ")]
    conf = [i for i, line in enumerate(out) if line.startswith("[conf:build] ")]
    assert len(cast) == 1 and len(conf) == 1 and conf[0] + 1 == mine[0] < cast[0] and out[cast[0] + 1].startswith("[opt:build] ")
    assert all("symbols of include/" in line for line in out[conf[0]:cast[0]])
    import scsfm_hip.rolling  # noqa: F401  (build() imports it)
    assert "scsfm_hip.rolling" in sys.modules
