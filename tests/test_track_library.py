"""libscsfm_track.so, the twenty-third library (scsfm_hip.libraries.ADDED): the row stands in the open-ended tuple, whose
length and contents no test pins, and REGISTRY covers every row; the header declares exactly the entry points; the library
builds with hipcc for gfx950 (no GPU needed), exports exactly them and carries the tree's source id; no other library's
source id sees csrc_track; bad arguments are rejected with -1 (sizes with 0) before any pointer is touched; no kernel uses
scratch or spills a register; build() reports the library directly ahead of cast's line, in cast's wording."""
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
ENTRY_POINTS = {"scsfm_track_abi_version", "scsfm_track_source_id", "scsfm_track_ws_bytes", "scsfm_track_init",
                "scsfm_track_poses", "scsfm_track_iterate"}


def test_the_row_is_registered_in_the_open_ended_tuple():
    row = libraries.find("track")
    assert row in libraries.ADDED and row in libraries.REGISTRY and row not in libraries.CATALOGUE
    assert libraries.REGISTRY[:len(libraries.CATALOGUE)] == libraries.CATALOGUE
    assert set(libraries.REGISTRY) == set(libraries.CATALOGUE) | set(libraries.ADDED)
    assert len({r.name for r in libraries.REGISTRY}) == len(libraries.REGISTRY)
    assert all(libraries.find(r.name) is r for r in libraries.REGISTRY)
    assert row.abi == 1 and row.tag == "track:build" and not row.tag.startswith("build")
    assert row.csrc.endswith("csrc_track") and row.header.endswith("scsfm_track.h")
    assert row.lib.endswith("libscsfm_track.so") and row.prefix == "scsfm_track_"
    assert "libscsfm_track.so" not in libraries.SUMMARY and "track" not in libraries.BY_NAME
    assert build.TRACK_LIB == row.lib and build.TRACK_CSRC == row.csrc and _lib.TRACK_HEADER == row.header
    assert _lib.TRACK_LIB_PATH == row.lib and _lib.TRACK_ABI_VERSION == 1 and callable(_lib.get_track)
    assert row.what in _lib.get_track.__doc__
    assert callable(build.build_track) and callable(build.track_deps) and callable(build.track_is_stale)
    assert [os.path.basename(p) for p in build.track_sources()] == ["scsfm_track.hip"]
    assert build.track_source_id() == build.lib_source_id("track")
    assert "ADDED" in libraries.__doc__ and "open-ended" in libraries.__doc__


def test_other_source_ids_do_not_see_csrc_track():
    ids = []
    for row in libraries.REGISTRY:
        if row.name == "track":
            continue
        deps = build.lib_deps(row.name)
        assert deps and not any("csrc_track" in p or "scsfm_track" in p for p in deps), row.name
        ids.append(build.lib_source_id(row.name))
    assert all(os.sep + "csrc_track" + os.sep in p or p.endswith("scsfm_track.h") or p == build.ICP_CORE
               for p in build.track_deps())
    assert build.ICP_CORE in build.track_deps()     # (the ICP core it shares with csrc_sim3, which belongs to no row)
    assert len(set(ids)) == len(ids) and build.track_source_id() not in ids


def test_header_declares_exactly_the_entry_points():
    decls = _lib.parse_header(_lib.TRACK_HEADER)
    assert set(decls) == ENTRY_POINTS
    assert len(decls["scsfm_track_init"][1]) == 6 and len(decls["scsfm_track_poses"][1]) == 4
    assert len(decls["scsfm_track_iterate"][1]) == 18 and decls["scsfm_track_ws_bytes"][0] is ctypes.c_size_t
    text = open(_lib.TRACK_HEADER).read()
    for word in ("CANDIDATE", "TERMS", "STATUS 1", "STATUS 2", "STATUS 0", "NORMALISE", "Shepperd", "butterfly",
                 "SCSFM_TRACK_PIVOT_EPS 1e-8"):
        assert word in text, word


def _lib_track():
    return _lib.CLib(build.build_track(verbose=False), _lib.TRACK_HEADER, _lib.TRACK_ABI_VERSION, "scsfm_track_")


@needs_hipcc
def test_track_library_builds_and_exports_its_header():
    path = build.build_track(verbose=False)
    assert path.endswith("libscsfm_track.so")
    assert build.binary_source_id(path) == build.track_source_id() and not build.track_is_stale()
    lib = _lib_track()
    assert lib.source_id() == build.track_source_id()
    assert lib._fn["scsfm_track_abi_version"]() == 1
    assert set(lib.decls) == ENTRY_POINTS
    nm = shutil.which("nm") or "/opt/rocm/llvm/bin/llvm-nm"
    syms = subprocess.run([nm, "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in syms.splitlines() if " T " in line and "scsfm" in line}
    assert exported == ENTRY_POINTS
    assert _lib.get_track().path == path


@needs_hipcc
def test_argument_errors_return_minus_one():
    lib = _lib_track()
    p = ctypes.c_void_p(4096)  # never dereferenced: every call below is rejected before anything is launched
    nan, inf, big = float("nan"), float("inf"), 2 ** 31 - 1
    ws_bytes = lib._fn["scsfm_track_ws_bytes"]
    assert ws_bytes(3, 12, 20) == 3 * 1 * 29 * 8 and ws_bytes(3, 37, 61) == 3 * 3 * 29 * 8
    assert ws_bytes(1, 32, 32) == 29 * 8 and ws_bytes(1, 1, 1025) == 2 * 29 * 8 and ws_bytes(64, 256, 832) == 64 * 208 * 232
    for dims in ((0, 12, 20), (3, 0, 20), (3, 12, -1), (1, 65536, 65536), (big, 1, 1), (big, big, big), (1024, 1024, 1024),
                 (2 ** 27, 1, 1)):
        assert ws_bytes(*dims) == 0, dims
    init, poses, iterate = (lib._fn["scsfm_track_" + k] for k in ("init", "poses", "iterate"))
    odd2, odd4 = ctypes.c_void_p(4098), ctypes.c_void_p(4100)
    for args in ((0, p, p, p, p), (-3, p, p, p, p), (2 ** 27, p, p, p, p), (2, None, p, p, p), (2, p, None, p, p),
                 (2, p, p, None, p), (2, p, p, p, None), (2, odd4, p, p, p), (2, p, odd2, p, p), (2, p, p, odd4, p),
                 (2, p, p, p, odd2)):
        assert init(*args, None) == -1, args
    for args in ((0, p, p), (-1, p, p), (2 ** 27, p, p), (2, None, p), (2, p, None), (2, odd4, p), (2, p, odd4)):
        assert poses(*args, None) == -1, args
    #       0  1  2  3      4        5    6          7    8  9  10        11         12       13     14   15  16
    #       V  H  W  depth  is_disp  near max_depth  ref  M  N  max_dist  min_pairs  n_iters  state  est  ws  report
    good = [3, 12, 20, p, 1, 0.0, 10.0, p, p, p, 0.3, 64, 10, p, p, p, p]
    for k, bad in ((0, 0), (0, -1), (1, 0), (2, -4), (1, 65536), (0, big), (2, big), (3, None), (3, odd2), (5, -0.01),
                   (5, nan), (5, inf), (6, 0.0), (6, -1.0), (6, nan), (6, inf), (7, None), (7, odd2), (8, None), (8, odd2),
                   (9, None), (9, odd2), (10, 0.0), (10, -0.1), (10, nan), (10, inf), (11, 5), (11, 0), (11, -1), (12, 0),
                   (12, -1), (12, 65), (13, None), (13, odd4), (14, None), (14, odd2), (15, None), (15, odd4), (16, None),
                   (16, odd4)):
        args = list(good)
        args[k] = bad
        if k == 1 and bad == 65536:
            args[2] = 65536   # H W past int
        assert iterate(*args, None) == -1, (k, bad)
    args = list(good)
    args[0], args[1], args[2] = 1024, 1024, 1024  # V 3 H W past int
    assert iterate(*args, None) == -1
    assert lib._fn["scsfm_track_source_id"](None, 64) == -1


@needs_hipcc
def test_no_kernel_spills_to_scratch(tmp_path):
    """The compiler's resource usage of the four kernels (read as tests/test_cast_library.py reads it): no scratch and no
    spilled register -- the 29 double accumulators of the sums and the 6 x 6 matrices of the solve live in registers."""
    out = tmp_path / "track.s"
    flags = [f for f in build.FLAGS if f not in ("-shared", "-fPIC")]
    (src,) = build.track_sources()
    subprocess.run([HIPCC, *flags, "-S", "--cuda-device-only", "-I", os.path.join(ROOT, "include"), "-o", str(out), src],
                   check=True, capture_output=True)
    text = open(out).read()
    kernels = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M)
    scratch = [int(x) for x in re.findall(r";\s*ScratchSize:\s*(\d+)", text)]
    spills = [int(x) for x in re.findall(r"\.[sv]gpr_spill_count:\s*(\d+)", text)]
    assert len(kernels) == 4 and len(scratch) == 4 and len(spills) == 8, (kernels, scratch, spills)
    for name in ("init_kernel", "poses_kernel", "accumulate_kernel", "solve_kernel"):
        assert sum(name in k for k in kernels) == 1, name
    assert scratch == [0] * 4 and not any(spills), (scratch, spills)


@needs_hipcc
def test_build_reports_the_library_directly_ahead_of_casts_line(capsys):
    """The line is in cast's wording: it does not contain "entry points resolved", does not start with "[build", and
    stands directly ahead of cast's line, which stays directly in front of opt's."""
    import sys
    sys.path.insert(0, ROOT)
    import __graft_entry__ as G
    G.build()
    out = capsys.readouterr().out.splitlines()
    mine = [i for i, line in enumerate(out) if line.startswith("[track:build] ")]
    assert len(mine) == 1
    assert out[mine[0]] == f"[track:build] {build.TRACK_LIB}: ABI 1, {len(ENTRY_POINTS)} symbols of include/scsfm_track.h"
    cast = [i for i, line in enumerate(out) if line.startswith("[cast:build] ")]
    assert len(cast) == 1 and mine[0] < cast[0] and out[cast[0] + 1].startswith("[opt:build] ")
    assert all("symbols of include/" in line for line in out[mine[0]:cast[0]])   # (only rows of ADDED in between)
    import scsfm_hip.tracking  # noqa: F401  (build() imports it)
    assert "scsfm_hip.tracking" in sys.modules
