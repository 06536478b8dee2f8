"""libscsfm_mesh.so, the twenty-first library (scsfm_hip.libraries.BEYOND): the row stands in a sixth tuple and leaves TABLE,
LATER, NEWER, ROWS, NEWEST, EVERY, NEXT, ALL and the keys of BY_NAME as they are, and LIBRARIES covers every row; the header
declares exactly the entry points; the library builds with hipcc for gfx950 (no GPU needed), exports exactly them and
carries the tree's source id; no other library's source id sees csrc_mesh; bad arguments are rejected with -1 (sizes with
0) before any pointer is touched; no kernel uses scratch or spills a register; build() reports the library directly
behind dgrad's line, in opt's, pw's and fuse's wording, which leaves every older pin of the output in place."""
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
ENTRY_POINTS = {"scsfm_mesh_abi_version", "scsfm_mesh_source_id", "scsfm_mesh_ws_bytes", "scsfm_mesh_count",
                "scsfm_mesh_vertices", "scsfm_mesh_triangles"}


def test_the_row_is_registered_in_a_sixth_tuple():
    assert [row.name for row in libraries.BEYOND] == ["mesh"]
    assert [row.name for row in libraries.NEXT] == ["fuse"]
    assert [row.name for row in libraries.NEWEST] == ["pw"] and [row.name for row in libraries.NEWER] == ["opt"]
    assert [row.name for row in libraries.LATER] == ["fbn"] and len(libraries.TABLE) == 16
    assert set(libraries.BY_NAME) == {r.name for r in libraries.TABLE} | {"fbn"}
    assert libraries.ROWS == libraries.TABLE + libraries.LATER + libraries.NEWER
    assert libraries.EVERY == libraries.ROWS + libraries.NEWEST
    assert libraries.ALL == libraries.EVERY + libraries.NEXT and len(libraries.ALL) == 20
    assert libraries.LIBRARIES == libraries.ALL + libraries.BEYOND and len(libraries.LIBRARIES) == 21
    assert len({r.name for r in libraries.LIBRARIES}) == 21
    row = libraries.find("mesh")
    assert row is libraries.BEYOND[0] and row.abi == 1 and row.tag == "mesh:build" and not row.tag.startswith("build")
    assert all(libraries.find(r.name) is r for r in libraries.LIBRARIES)
    assert row.csrc.endswith("csrc_mesh") and row.header.endswith("scsfm_mesh.h")
    assert row.lib.endswith("libscsfm_mesh.so") and row.prefix == "scsfm_mesh_"
    for text in (libraries.SUMMARY, build.__doc__, _lib.__doc__):
        assert "libscsfm_mesh.so" in text and "libscsfm_fuse.so" in text
    assert len(libraries.SUMMARY.splitlines()) == 21
    assert build.MESH_LIB == row.lib and build.MESH_CSRC == row.csrc and _lib.MESH_HEADER == row.header
    assert _lib.MESH_LIB_PATH == row.lib and _lib.MESH_ABI_VERSION == 1 and callable(_lib.get_mesh)
    assert row.what in _lib.get_mesh.__doc__
    assert callable(build.build_mesh) and callable(build.mesh_deps) and callable(build.mesh_is_stale)
    assert [os.path.basename(p) for p in build.mesh_sources()] == ["scsfm_mesh.hip"]
    assert build.mesh_source_id() == build.lib_source_id("mesh")


def test_other_source_ids_do_not_see_csrc_mesh():
    ids = []
    for row in libraries.ALL:
        deps = build.lib_deps(row.name)
        assert deps and not any("csrc_mesh" in p or "scsfm_mesh" in p for p in deps), row.name
        ids.append(build.lib_source_id(row.name))
    assert all(os.sep + "csrc_mesh" + os.sep in p or p.endswith("scsfm_mesh.h") for p in build.mesh_deps())
    assert len(set(ids)) == 20 and build.mesh_source_id() not in ids


def test_header_declares_exactly_the_entry_points_and_the_orientation_table():
    decls = _lib.parse_header(_lib.MESH_HEADER)
    assert set(decls) == ENTRY_POINTS
    assert len(decls["scsfm_mesh_count"][1]) == 8 and len(decls["scsfm_mesh_vertices"][1]) == 16
    assert len(decls["scsfm_mesh_triangles"][1]) == 12
    # the header's table of swapped cases is what the oracle's exact integer evaluation gives
    import mesh_oracle as MO
    text = open(_lib.MESH_HEADER).read()
    macro = re.search(r"#define SCSFM_MESH_FLIP\(tet\) \(\(0x([0-9a-f]+) >> \(tet\)\) & 1 \? 0x([0-9a-f]+) : 0x([0-9a-f]+)\)", text)
    which, odd, even = (int(g, 16) for g in macro.groups())
    assert f"0x{even:04x} for the tetrahedra 0, 3, 4,  0x{odd:04x} for 1, 2, 5" in text and which == 0b100110
    for ti, tet in enumerate(MO.TETS):
        table = odd if (which >> ti) & 1 else even
        for c4 in range(1, 15):
            inside = {k for j, k in enumerate(tet) if (c4 >> j) & 1}
            I, O = [k for k in tet if k in inside], [k for k in tet if k not in inside]
            if len(I) == 2:
                first = [(I[0], O[0]), (I[0], O[1]), (I[1], O[1])]
            else:
                first = [(I[0], o) for o in O] if len(I) == 1 else [(i, O[0]) for i in I]
            plain = [(min(p, q), max(p, q)) for p, q in first]
            got = MO.case_triangles(tet, inside)[0]
            assert got in (plain, [plain[0], plain[2], plain[1]])
            assert (got != plain) == bool((table >> c4) & 1), (ti, c4)


def _lib_mesh():
    return _lib.CLib(build.build_mesh(verbose=False), _lib.MESH_HEADER, _lib.MESH_ABI_VERSION, "scsfm_mesh_")


@needs_hipcc
def test_mesh_library_builds_and_exports_its_header():
    path = build.build_mesh(verbose=False)
    assert path.endswith("libscsfm_mesh.so")
    assert build.binary_source_id(path) == build.mesh_source_id() and not build.mesh_is_stale()
    lib = _lib_mesh()
    assert lib.source_id() == build.mesh_source_id()
    assert lib._fn["scsfm_mesh_abi_version"]() == 1
    assert set(lib.decls) == ENTRY_POINTS
    nm = shutil.which("nm") or "/opt/rocm/llvm/bin/llvm-nm"
    syms = subprocess.run([nm, "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in syms.splitlines() if " T " in line and "scsfm" in line}
    assert exported == ENTRY_POINTS
    assert _lib.get_mesh().path == path


@needs_hipcc
def test_argument_errors_return_minus_one():
    lib = _lib_mesh()
    p = ctypes.c_void_p(4096)  # never dereferenced: every call below is rejected before anything is launched
    nan, inf, big = float("nan"), float("inf"), 2 ** 31 - 1
    ws_bytes = lib._fn["scsfm_mesh_ws_bytes"]
    up = lambda n: (n + 15) // 16 * 16  # noqa: E731
    assert ws_bytes(37, 18, 29) == up(16 + 24 * 19 + 5 * 37 * 18 * 29)
    assert ws_bytes(1024, 1024, 512) == 16 + 24 * 2 ** 19 + 5 * 2 ** 29 and ws_bytes(1, 1, 1) == 48
    for dims in ((0, 4, 4), (4, -1, 4), (4, 4, 0), (1024, 1024, 513), (big, 1, 1), (big, big, big), (65536, 65536, 1),
                 (2 ** 29 + 1, 1, 1), (1, 2 ** 15, 2 ** 15)):
        assert ws_bytes(*dims) == 0, dims
    count, vertices, triangles = (lib._fn["scsfm_mesh_" + k] for k in ("count", "vertices", "triangles"))
    n = ws_bytes(8, 6, 5)
    odd4, odd2 = ctypes.c_void_p(4100), ctypes.c_void_p(4098)
    #         nx ny nz volume min_weight ws ws_bytes
    good_c = [8, 6, 5, p, 1.0, p, n]
    for k, bad in ((0, 0), (2, -1), (0, 2 ** 30), (3, None), (3, odd2), (4, 0.5), (4, 0.0), (4, nan), (4, inf), (4, -inf),
                   (5, None), (5, odd4), (6, n - 4), (6, 0)):
        args = list(good_c)
        args[k] = bad
        assert count(*args, None) == -1, (k, bad)
    #         0  1  2  3    4    5    6     7      8          9  10       11         12       13  14
    #         nx ny nz ox   oy   oz   voxel volume min_weight ws ws_bytes n_vertices capacity xyz rgb
    good_v = [8, 6, 5, 0.0, 0.0, 0.0, 0.1, p, 1.0, p, n, 10, 10, p, p]
    for k, bad in ((0, 0), (1, 2 ** 30), (3, nan), (4, inf), (5, -inf), (6, 0.0), (6, -0.1), (6, nan), (6, inf), (7, None),
                   (7, odd2), (8, 0.99), (8, nan), (9, None), (9, odd4), (10, n - 1), (11, 2 ** 31), (11, 7 * 2 ** 29),
                   (12, -1), (13, None), (13, odd2), (14, None)):
        args = list(good_v)
        args[k] = bad
        assert vertices(*args, None) == -1, (k, bad)
    #         0  1  2  3      4          5  6        7          8           9        10
    #         nx ny nz volume min_weight ws ws_bytes n_vertices n_triangles capacity tri
    good_t = [8, 6, 5, p, 1.0, p, n, 10, 10, 10, p]
    for k, bad in ((0, -8), (2, 2 ** 30), (3, None), (4, 0.5), (4, nan), (5, None), (5, odd4), (6, n - 16), (7, 2 ** 31),
                   (8, 2 ** 31), (8, 12 * 2 ** 29), (9, -1), (10, None), (10, odd2)):
        args = list(good_t)
        args[k] = bad
        assert triangles(*args, None) == -1, (k, bad)
    args = list(good_t)
    args[9], args[10] = 0, None   # a capacity of 0: nothing to write, nothing launched
    assert triangles(*args, None) == 0
    assert lib._fn["scsfm_mesh_source_id"](None, 64) == -1


@needs_hipcc
def test_no_kernel_spills_to_scratch(tmp_path):
    """The compiler's resource usage of the four kernels (read as tests/test_fuse_library.py reads it): no scratch and no
    spilled register."""
    out = tmp_path / "mesh.s"
    flags = [f for f in build.FLAGS if f not in ("-shared", "-fPIC")]
    (src,) = build.mesh_sources()
    subprocess.run([HIPCC, *flags, "-S", "--cuda-device-only", "-I", os.path.join(ROOT, "include"), "-o", str(out), src],
                   check=True, capture_output=True)
    text = open(out).read()
    kernels = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M)
    scratch = [int(x) for x in re.findall(r";\s*ScratchSize:\s*(\d+)", text)]
    spills = [int(x) for x in re.findall(r"\.[sv]gpr_spill_count:\s*(\d+)", text)]
    assert len(kernels) == 4 and len(scratch) == 4 and len(spills) == 8, (kernels, scratch, spills)
    assert sum("mesh_kernel" in k for k in kernels) == 3 and sum("scan_kernel" in k for k in kernels) == 1
    assert scratch == [0] * 4 and not any(spills), (scratch, spills)


@needs_hipcc
def test_build_reports_the_library_directly_behind_dgrad(capsys):
    """The place the older pins leave: opt, pw, fbn, fuse and dgrad stay on consecutive lines, seventeen lines END in
    "entry points resolved" (this one carries "(ABI 1)"), ten start with "[build", snip stands directly ahead of vis,
    and vis and prep come last."""
    import sys
    sys.path.insert(0, ROOT)
    import __graft_entry__ as G
    G.build()
    out = capsys.readouterr().out.splitlines()
    mine = [i for i, line in enumerate(out) if line.startswith("[mesh:build] ")]
    assert len(mine) == 1
    assert out[mine[0]] == f"[mesh:build] {build.MESH_LIB}: {len(ENTRY_POINTS)} entry points resolved (ABI 1)"
    first = min(i for i, line in enumerate(out) if "entry points resolved" in line)
    tags = [line.split("]")[0] + "]" for line in out[first:first + 7]]
    assert tags == ["[opt:build]", "[pw:build]", "[fbn:build]", "[fuse:build]", "[dgrad:build]", "[mesh:build]",
                    "[vlog:build]"]
    assert len([line for line in out if line.endswith("entry points resolved")]) == 17
    assert len([line for line in out if "entry points resolved" in line]) == 21
    assert len([line for line in out if line.startswith("[build")]) == 10
    vis = [i for i, line in enumerate(out) if line.startswith("[build:vis] ")][0]
    assert "libscsfm_snip.so" in out[vis - 1]
    assert out[-2].startswith("[build:vis] ") and out[-1].startswith("[build:prep] ")
