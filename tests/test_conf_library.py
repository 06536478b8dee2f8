"""libscsfm_conf.so, the twenty-fourth library (scsfm_hip.libraries.ADDED): the row stands in the open-ended tuple and
REGISTRY covers it; the header declares exactly the entry points; the library builds with hipcc for gfx950 (no GPU needed),
exports exactly them and carries the tree's source id; no other library's source id sees csrc_conf, and csrc_conf includes
nothing of another library; bad arguments are rejected with -1 before any pointer is touched; no kernel uses scratch or
spills a register; build() reports the library ahead of cast's line, in cast's wording."""
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
ENTRY_POINTS = {"scsfm_conf_abi_version", "scsfm_conf_source_id", "scsfm_conf_pairs", "scsfm_conf_weights",
                "scsfm_conf_integrate"}


def test_the_row_is_registered_in_the_open_ended_tuple():
    row = libraries.find("conf")
    assert row in libraries.ADDED and row in libraries.REGISTRY and row not in libraries.CATALOGUE
    assert libraries.REGISTRY == libraries.CATALOGUE + libraries.ADDED and libraries.ADDED[0].name == "track"
    assert len({r.name for r in libraries.REGISTRY}) == len(libraries.REGISTRY) >= 24
    assert row.abi == 1 and row.tag == "conf:build" and not row.tag.startswith("build")
    assert row.csrc.endswith("csrc_conf") and row.header.endswith("scsfm_conf.h")
    assert row.lib.endswith("libscsfm_conf.so") and row.prefix == "scsfm_conf_"
    assert "libscsfm_conf.so" not in libraries.SUMMARY and "conf" not in libraries.BY_NAME
    for text in (libraries.SINCE, build.__doc__, _lib.__doc__):     # (the rows since SUMMARY was fixed are listed behind it)
        assert "libscsfm_conf.so" in text and "libscsfm_track.so" in text and "include/scsfm_conf.h" in text
    assert build.CONF_LIB == row.lib and build.CONF_CSRC == row.csrc and _lib.CONF_HEADER == row.header
    assert _lib.CONF_LIB_PATH == row.lib and _lib.CONF_ABI_VERSION == 1 and callable(_lib.get_conf)
    assert row.what in _lib.get_conf.__doc__
    assert callable(build.build_conf) and callable(build.conf_deps) and callable(build.conf_is_stale)
    assert [os.path.basename(p) for p in build.conf_sources()] == ["scsfm_conf.hip"]
    assert build.conf_source_id() == build.lib_source_id("conf")


def test_source_ids_are_per_library():
    ids = []
    for row in libraries.REGISTRY:
        if row.name == "conf":
            continue
        deps = build.lib_deps(row.name)
        assert deps and not any("csrc_conf" in p or "scsfm_conf" in p for p in deps), row.name
        ids.append(build.lib_source_id(row.name))
    assert all(os.sep + "csrc_conf" + os.sep in p or p.endswith("scsfm_conf.h") for p in build.conf_deps())
    assert len(set(ids)) == len(ids) and build.conf_source_id() not in ids
    # the integration is restated, not shared: the source includes its own header and no other of the project's
    (src,) = build.conf_sources()
    mine = re.findall(r'#include\s+"([^"]+)"', open(src).read())
    assert mine == ["scsfm_conf.h"]
    assert not re.findall(r'#include\s+"', open(_lib.CONF_HEADER).read())


def test_header_declares_exactly_the_entry_points():
    decls = _lib.parse_header(_lib.CONF_HEADER)
    assert set(decls) == ENTRY_POINTS
    assert len(decls["scsfm_conf_pairs"][1]) == 6 and len(decls["scsfm_conf_weights"][1]) == 13
    # scsfm_fuse_integrate's arguments and the weight after the depth
    fuse = _lib.parse_header(_lib.FUSE_HEADER)["scsfm_fuse_integrate"][1]
    mine = decls["scsfm_conf_integrate"][1]
    assert len(mine) == len(fuse) + 1 == 21 and mine[:16] == fuse[:16] and mine[16] is ctypes.c_void_p and mine[17:] == fuse[16:]
    text = open(_lib.CONF_HEADER).read()
    for word in ("SCSFM_CONF_MAX_RADIUS 4", "true floor", "-radius .. -1, 1 .. radius", "sixteen zeros", "best = m > best",
                 "min(w + c, max_weight)", "fl(tn c)", "fl(col c)", "c > 0 && c <= 1"):
        assert word in text, word


def _lib_conf():
    return _lib.CLib(build.build_conf(verbose=False), _lib.CONF_HEADER, _lib.CONF_ABI_VERSION, "scsfm_conf_")


@needs_hipcc
def test_conf_library_builds_and_exports_its_header():
    path = build.build_conf(verbose=False)
    assert path.endswith("libscsfm_conf.so")
    assert build.binary_source_id(path) == build.conf_source_id() and not build.conf_is_stale()
    lib = _lib_conf()
    assert lib.source_id() == build.conf_source_id()
    assert lib._fn["scsfm_conf_abi_version"]() == 1
    assert set(lib.decls) == ENTRY_POINTS
    nm = shutil.which("nm") or "/opt/rocm/llvm/bin/llvm-nm"
    syms = subprocess.run([nm, "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in syms.splitlines() if " T " in line and "scsfm" in line}
    assert exported == ENTRY_POINTS
    assert _lib.get_conf().path == path


@needs_hipcc
def test_argument_errors_return_minus_one():
    lib = _lib_conf()
    p = ctypes.c_void_p(4096)  # never dereferenced: every call below is rejected before anything is launched
    odd2, odd4 = ctypes.c_void_p(4098), ctypes.c_void_p(4100)
    nan, inf, big = float("nan"), float("inf"), 2 ** 31 - 1
    pairs, weights, integrate = (lib._fn["scsfm_conf_" + k] for k in ("pairs", "weights", "integrate"))
    #            n  radius  c2w  K  pair
    for args in ((0, 1, p, p, p), (-2, 1, p, p, p), (3, 0, p, p, p), (3, 5, p, p, p), (3, -1, p, p, p), (big, 1, p, p, p),
                 (2 ** 24, 4, p, p, p), (3, 1, None, p, p), (3, 1, p, None, p), (3, 1, p, p, None), (3, 1, odd4, p, p),
                 (3, 1, p, odd2, p), (3, 1, p, p, odd2)):
        assert pairs(*args, None) == -1, args
    #       0  1       2   3   4      5        6     7          8          9      10      11
    #       n  radius  H   W   depth  is_disp  pair  max_depth  min_views  floor  reduce  weight
    good = [3, 1, 12, 20, p, 1, p, 10.0, 1, 0.0, 0, p]
    for k, bad in ((0, 0), (0, -1), (1, 0), (1, 5), (2, 0), (3, -4), (0, big), (2, big), (4, None), (4, odd2), (6, None),
                   (6, odd2), (7, 0.0), (7, -1.0), (7, nan), (7, inf), (8, 0), (8, -1), (9, -0.01), (9, 1.01), (9, nan),
                   (9, inf), (10, 2), (10, -1), (11, None), (11, odd2)):
        args = list(good)
        args[k] = bad
        assert weights(*args, None) == -1, (k, bad)
    args = list(good)
    args[0], args[2], args[3] = 1024, 2048, 1024   # n H W past int
    assert weights(*args, None) == -1
    args[0], args[2], args[3] = 1, 65536, 65536    # H W past int
    assert weights(*args, None) == -1
    #       0   1   2   3    4    5    6      7      8     9          10          11 12 13 14   15     16      17       18     19
    #       nx  ny  nz  ox   oy   oz   voxel  trunc  near  max_depth  max_weight  F  H  W  cam  depth  weight  is_disp  image  volume
    good = [37, 19, 22, 0.0, 0.0, 0.0, 0.1, 0.3, 0.0, 10.0, 64.0, 5, 12, 20, p, p, p, 1, p, p]
    for k, bad in ((0, 0), (1, -1), (2, 0), (0, big), (3, nan), (4, inf), (5, -inf), (6, 0.0), (6, nan), (7, 0.0), (7, inf),
                   (8, -0.1), (8, nan), (9, 0.0), (9, nan), (10, 0.5), (10, nan), (10, inf), (11, 0), (11, -1), (12, 0),
                   (13, 0), (14, None), (14, odd2), (15, None), (15, odd2), (16, None), (16, odd2), (18, odd2), (19, None),
                   (19, odd2)):
        args = list(good)
        args[k] = bad
        assert integrate(*args, None) == -1, (k, bad)
    args = list(good)
    args[0], args[1], args[2] = 1024, 1024, 1024   # more than 2^29 voxels
    assert integrate(*args, None) == -1
    args = list(good)
    args[11], args[12], args[13] = 1024, 1024, 1024   # F 3 H W past int
    assert integrate(*args, None) == -1
    assert lib._fn["scsfm_conf_source_id"](None, 64) == -1


@needs_hipcc
def test_no_kernel_spills_to_scratch(tmp_path):
    """The compiler's resource usage of the seven kernels (read as tests/test_track_library.py reads it): no scratch and
    no spilled register -- a pixel's sums and a voxel's five values and its frames live in registers."""
    out = tmp_path / "conf.s"
    flags = [f for f in build.FLAGS if f not in ("-shared", "-fPIC")]
    (src,) = build.conf_sources()
    subprocess.run([HIPCC, *flags, "-S", "--cuda-device-only", "-I", os.path.join(ROOT, "include"), "-o", str(out), src],
                   check=True, capture_output=True)
    text = open(out).read()
    kernels = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M)
    scratch = [int(x) for x in re.findall(r";\s*ScratchSize:\s*(\d+)", text)]
    spills = [int(x) for x in re.findall(r"\.[sv]gpr_spill_count:\s*(\d+)", text)]
    assert len(kernels) == 7 and len(scratch) == 7 and len(spills) == 14, (kernels, scratch, spills)
    for name, copies in (("pairs_kernel", 1), ("weights_kernel", 2), ("integrate_kernel", 4)):
        assert sum(name in k for k in kernels) == copies, name
    assert scratch == [0] * 7 and not any(spills), (scratch, spills)


@needs_hipcc
def test_build_reports_the_library_ahead_of_casts_line(capsys):
    """The line is in cast's wording: it does not contain "entry points resolved", does not start with "[build", and
    stands behind track's line and ahead of cast's, which stays directly in front of opt's."""
    import sys
    sys.path.insert(0, ROOT)
    import __graft_entry__ as G
    G.build()
    out = capsys.readouterr().out.splitlines()
    mine = [i for i, line in enumerate(out) if line.startswith("[conf:build] ")]
    assert len(mine) == 1
    assert out[mine[0]] == f"[conf:build] {build.CONF_LIB}: ABI 1, {len(ENTRY_POINTS)} symbols of include/scsfm_conf.h"
    cast = [i for i, line in enumerate(out) if line.startswith("[cast:build] ")]
    track = [i for i, line in enumerate(out) if line.startswith("[track:build] ")]
    assert len(cast) == 1 and len(track) == 1 and track[0] < mine[0] < cast[0] and out[cast[0] + 1].startswith("[opt:build] ")
    assert all("symbols of include/" in line for line in out[track[0]:cast[0]])
    import scsfm_hip.confidence  # noqa: F401  (build() imports it)
    assert "scsfm_hip.confidence" in sys.modules
