"""libscsfm_sim3.so, the twenty-sixth library (scsfm_hip.libraries.ADDED): the row stands in the open-ended tuple and
REGISTRY covers it; the header declares exactly the entry points; the library builds with hipcc for gfx950 (no GPU needed),
exports exactly them and carries the tree's source id; no other library's source id sees csrc_sim3, and csrc_sim3 includes
nothing of another library (the ICP core it shares with csrc_track belongs to neither); bad arguments are rejected with
-1 (sizes with 0) before any pointer is touched; no kernel uses scratch or spills a register; build() reports the library
among ADDED's lines, ahead of cast's, in cast's wording."""
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
ENTRY_POINTS = {"scsfm_sim3_abi_version", "scsfm_sim3_source_id", "scsfm_sim3_ws_bytes", "scsfm_sim3_init",
                "scsfm_sim3_poses", "scsfm_sim3_iterate", "scsfm_sim3_scale"}


def test_the_row_is_registered_in_the_open_ended_tuple():
    row = libraries.find("sim3")
    assert row in libraries.ADDED and row in libraries.REGISTRY and row not in libraries.CATALOGUE
    assert libraries.REGISTRY == libraries.CATALOGUE + libraries.ADDED
    assert [r.name for r in libraries.ADDED[:4]] == ["track", "conf", "roll", "sim3"]
    assert len({r.name for r in libraries.REGISTRY}) == len(libraries.REGISTRY) >= 26
    assert row.abi == 1 and row.tag == "sim3:build" and not row.tag.startswith("build")
    assert row.csrc.endswith("csrc_sim3") and row.header.endswith("scsfm_sim3.h")
    assert row.lib.endswith("libscsfm_sim3.so") and row.prefix == "scsfm_sim3_"
    assert "libscsfm_sim3.so" not in libraries.SUMMARY and "sim3" not in libraries.BY_NAME
    for text in (libraries.SINCE, build.__doc__, _lib.__doc__):     # (the rows since SUMMARY was fixed are listed behind it)
        assert "libscsfm_sim3.so" in text and "libscsfm_track.so" in text and "include/scsfm_sim3.h" in text
    assert build.SIM3_LIB == row.lib and build.SIM3_CSRC == row.csrc and _lib.SIM3_HEADER == row.header
    assert _lib.SIM3_LIB_PATH == row.lib and _lib.SIM3_ABI_VERSION == 1 and callable(_lib.get_sim3)
    assert row.what in _lib.get_sim3.__doc__
    assert callable(build.build_sim3) and callable(build.sim3_deps) and callable(build.sim3_is_stale)
    assert [os.path.basename(p) for p in build.sim3_sources()] == ["scsfm_sim3.hip"]
    assert build.sim3_source_id() == build.lib_source_id("sim3")


def test_source_ids_are_per_library():
    ids = []
    for row in libraries.REGISTRY:
        if row.name == "sim3":
            continue
        deps = build.lib_deps(row.name)
        assert deps and not any("csrc_sim3" in p or "scsfm_sim3" in p for p in deps), row.name
        ids.append(build.lib_source_id(row.name))
    assert all(os.sep + "csrc_sim3" + os.sep in p or p.endswith("scsfm_sim3.h") or p == build.ICP_CORE
               for p in build.sim3_deps())
    assert build.ICP_CORE in build.sim3_deps()
    assert len(set(ids)) == len(ids) and build.sim3_source_id() not in ids
    # the source includes its own header and the ICP core it shares with csrc_track, and no other of the project's
    (src,) = build.sim3_sources()
    assert re.findall(r'#include\s+"([^"]+)"', open(src).read()) == ["scsfm_sim3.h", "../csrc_icp/scsfm_icp.h"]
    assert not re.findall(r'#include\s+"', open(_lib.SIM3_HEADER).read())
    # the core belongs to no row: exactly the two trackers' ids cover it, and it includes nothing of the project's
    assert os.path.samefile(build.ICP_CORE, os.path.join(os.path.dirname(src), "../csrc_icp/scsfm_icp.h"))
    for row in libraries.REGISTRY:
        assert (build.ICP_CORE in build.lib_deps(row.name)) == (row.name in ("track", "sim3")), row.name
    core = open(build.ICP_CORE).read()
    assert not re.findall(r'#include\s+"', core) and not re.findall(r"#include\s+<[^>]*scsfm", core)
    every = [build.lib_source_id(row.name) for row in libraries.REGISTRY]
    assert len(set(every)) == len(every)


def test_header_declares_exactly_the_entry_points():
    decls = _lib.parse_header(_lib.SIM3_HEADER)
    assert set(decls) == ENTRY_POINTS
    i, f, d, p, z = ctypes.c_int, ctypes.c_float, ctypes.c_double, ctypes.c_void_p, ctypes.c_size_t
    track = _lib.parse_header(_lib.TRACK_HEADER)
    assert decls["scsfm_sim3_ws_bytes"] == (z, [i, i, i]) == track["scsfm_track_ws_bytes"]
    # track's arguments with the scales: scale0 behind c2w and sigma_f behind est; scale behind c2w; min_scale_pivot behind
    # min_pairs and sigma_f behind est
    init, poses, iterate = (track["scsfm_track_" + k][1] for k in ("init", "poses", "iterate"))
    assert decls["scsfm_sim3_init"] == (i, init[:2] + [p] + init[2:5] + [p] + init[5:])
    assert decls["scsfm_sim3_poses"] == (i, poses[:3] + [p] + poses[3:])
    assert decls["scsfm_sim3_iterate"] == (i, iterate[:12] + [d] + iterate[12:15] + [p] + iterate[15:])
    assert len(decls["scsfm_sim3_iterate"][1]) == 20
    assert decls["scsfm_sim3_scale"] == (i, [i, i, i, p, i, p, p, p])
    text = open(_lib.SIM3_HEADER).read()
    for word in ("CANDIDATE", "TERMS", "STATUS 0", "STATUS 1", "STATUS 2", "STATUS 3", "HELD", "NORMALISE", "Shepperd",
                 "butterfly", "SCSFM_SIM3_PIVOT_EPS 1e-8", "SCSFM_SIM3_STATE 8", "SCSFM_SIM3_SUMS 37",
                 "SCSFM_SIM3_REPORT 6", "d = fl(sigma_f[v] d0)", "fl(fl(sigma fl(1 + h)) / fl(1 - h))",
                 "fl(min_scale_pivot top)", "z_6 > -1 && z_6 < 1", "the term of\n *    k = 6 is not formed"):
        assert word in text, word
    for name, value in (("STATE", 8), ("RECORD", 16), ("SUMS", 37), ("TILE", 1024), ("REPORT", 6), ("MAX_ITERS", 64)):
        assert re.search(rf"#define SCSFM_SIM3_{name} {value}\b", text), name


def _lib_sim3():
    return _lib.CLib(build.build_sim3(verbose=False), _lib.SIM3_HEADER, _lib.SIM3_ABI_VERSION, "scsfm_sim3_")


@needs_hipcc
def test_sim3_library_builds_and_exports_its_header():
    path = build.build_sim3(verbose=False)
    assert path.endswith("libscsfm_sim3.so")
    assert build.binary_source_id(path) == build.sim3_source_id() and not build.sim3_is_stale()
    lib = _lib_sim3()
    assert lib.source_id() == build.sim3_source_id()
    assert lib._fn["scsfm_sim3_abi_version"]() == 1
    assert set(lib.decls) == ENTRY_POINTS
    nm = shutil.which("nm") or "/opt/rocm/llvm/bin/llvm-nm"
    syms = subprocess.run([nm, "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in syms.splitlines() if " T " in line and "scsfm" in line}
    assert exported == ENTRY_POINTS
    assert _lib.get_sim3().path == path


@needs_hipcc
def test_argument_errors_return_minus_one():
    lib = _lib_sim3()
    p = ctypes.c_void_p(4096)  # never dereferenced: every call below is rejected before anything is launched
    nan, inf, big = float("nan"), float("inf"), 2 ** 31 - 1
    ws_bytes = lib._fn["scsfm_sim3_ws_bytes"]
    assert ws_bytes(3, 12, 20) == 3 * 1 * 37 * 8 and ws_bytes(3, 37, 61) == 3 * 3 * 37 * 8
    assert ws_bytes(1, 32, 32) == 37 * 8 and ws_bytes(1, 1, 1025) == 2 * 37 * 8 and ws_bytes(64, 256, 832) == 64 * 208 * 296
    for dims in ((0, 12, 20), (3, 0, 20), (3, 12, -1), (1, 65536, 65536), (big, 1, 1), (big, big, big), (1024, 1024, 1024),
                 (2 ** 27, 1, 1)):
        assert ws_bytes(*dims) == 0, dims
    init, poses, iterate, scale = (lib._fn["scsfm_sim3_" + k] for k in ("init", "poses", "iterate", "scale"))
    odd2, odd4 = ctypes.c_void_p(4098), ctypes.c_void_p(4100)
    #       V  c2w  scale0  K  state  est  sigma_f
    good = [2, p, p, p, p, p, p]
    for k, bad in ((0, 0), (0, -3), (0, 2 ** 27), (1, None), (2, None), (3, None), (4, None), (5, None), (6, None),
                   (1, odd4), (2, odd4), (3, odd2), (4, odd4), (5, odd2), (6, odd2)):
        args = list(good)
        args[k] = bad
        assert init(*args, None) == -1, (k, bad)
    for args in ((0, p, p, p), (-1, p, p, p), (2 ** 27, p, p, p), (2, None, p, p), (2, p, None, p), (2, p, p, None),
                 (2, odd4, p, p), (2, p, odd4, p), (2, p, p, odd4)):
        assert poses(*args, None) == -1, args
    #       0  1   2   3      4        5    6          7    8  9  10        11         12               13       14
    #       V  H   W   depth  is_disp  near max_depth  ref  M  N  max_dist  min_pairs  min_scale_pivot  n_iters  state
    #       15   16       17  18
    #       est  sigma_f  ws  report
    good = [3, 12, 20, p, 1, 0.0, 10.0, p, p, p, 0.3, 64, 2e-3, 10, p, p, p, p, p]
    for k, bad in ((0, 0), (0, -1), (1, 0), (2, -4), (1, 65536), (0, big), (2, big), (3, None), (3, odd2), (5, -0.01),
                   (5, nan), (5, inf), (6, 0.0), (6, -1.0), (6, nan), (6, inf), (7, None), (7, odd2), (8, None), (8, odd2),
                   (9, None), (9, odd2), (10, 0.0), (10, -0.1), (10, nan), (10, inf), (11, 6), (11, 0), (11, -1),
                   (12, 0.0), (12, -2e-3), (12, nan), (12, -inf), (13, 0), (13, -1), (13, 65), (14, None), (14, odd4),
                   (15, None), (15, odd2), (16, None), (16, odd2), (17, None), (17, odd4), (18, None), (18, odd4)):
        args = list(good)
        args[k] = bad
        if k == 1 and bad == 65536:
            args[2] = 65536   # H W past int
        assert iterate(*args, None) == -1, (k, bad)
    args = list(good)
    args[0], args[1], args[2] = 1024, 1024, 1024  # V 3 H W past int
    assert iterate(*args, None) == -1
    #       V  H   W   depth  is_disp  sigma_f  out
    good = [3, 12, 20, p, 1, p, p]
    for k, bad in ((0, 0), (0, -1), (1, 0), (2, -4), (1, 65536), (0, big), (3, None), (3, odd2), (5, None), (5, odd2),
                   (6, None), (6, odd2)):
        args = list(good)
        args[k] = bad
        if k == 1 and bad == 65536:
            args[2] = 65536
        assert scale(*args, None) == -1, (k, bad)
    assert scale(2048, 1024, 1024, p, 1, p, p, None) == -1       # V H W past int
    assert lib._fn["scsfm_sim3_source_id"](None, 64) == -1


@needs_hipcc
def test_no_kernel_spills_to_scratch(tmp_path):
    """The compiler's resource usage of the five kernels (read as tests/test_track_library.py reads it): no scratch and no
    spilled register -- the 37 double accumulators of the sums and the 7 x 7 matrices of the solve live in registers."""
    out = tmp_path / "sim3.s"
    flags = [f for f in build.FLAGS if f not in ("-shared", "-fPIC")]
    (src,) = build.sim3_sources()
    subprocess.run([HIPCC, *flags, "-S", "--cuda-device-only", "-I", os.path.join(ROOT, "include"), "-o", str(out), src],
                   check=True, capture_output=True)
    text = open(out).read()
    kernels = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M)
    scratch = [int(x) for x in re.findall(r";\s*ScratchSize:\s*(\d+)", text)]
    spills = [int(x) for x in re.findall(r"\.[sv]gpr_spill_count:\s*(\d+)", text)]
    vgprs = [int(x) for x in re.findall(r";\s*NumVgprs:\s*(\d+)", text)]
    print(dict(zip(kernels, vgprs)))
    assert len(kernels) == 5 and len(scratch) == 5 and len(spills) == 10, (kernels, scratch, spills)
    for name in ("init_kernel", "poses_kernel", "accumulate_kernel", "solve_kernel", "scale_kernel"):
        assert sum(name in k for k in kernels) == 1, name
    assert scratch == [0] * 5 and not any(spills), (scratch, spills)
    # the streaming kernel's wide path is one 16-byte load and one 16-byte store
    (name,) = [k for k in kernels if "scale_kernel" in k]
    body = text[text.index(name + ":"):]
    body = body[:body.index(".amdhsa_kernel")]
    assert len(re.findall(r"global_load_dwordx4", body)) == 1 and len(re.findall(r"global_store_dwordx4", body)) == 1


@needs_hipcc
def test_build_reports_the_library_among_addeds_lines_ahead_of_casts(capsys):
    """The line is in cast's wording: it does not contain "entry points resolved", does not start with "[build", and
    stands directly behind roll's line and ahead of cast's, which stays directly in front of opt's."""
    import sys
    sys.path.insert(0, ROOT)
    import __graft_entry__ as G
    G.build()
    out = capsys.readouterr().out.splitlines()
    mine = [i for i, line in enumerate(out) if line.startswith("[sim3:build] ")]
    assert len(mine) == 1
    assert out[mine[0]] == f"[sim3:build] {build.SIM3_LIB}: ABI 1, {len(ENTRY_POINTS)} symbols of include/scsfm_sim3.h"
    cast = [i for i, line in enumerate(out) if line.startswith("[cast:build] ")]
    roll = [i for i, line in enumerate(out) if line.startswith("[roll:build] ")]
    assert len(cast) == 1 and len(roll) == 1 and roll[0] + 1 == mine[0] < cast[0] and out[cast[0] + 1].startswith("[opt:build] ")
    assert all("symbols of include/" in line for line in out[roll[0]:cast[0] + 1])
    import scsfm_hip.similarity  # noqa: F401  (build() imports it)
    assert "scsfm_hip.similarity" in sys.modules
