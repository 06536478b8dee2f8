"""libscsfm_pw.so, the nineteenth library (scsfm_hip.libraries.NEWEST): the row stands in a fourth tuple and leaves TABLE,
LATER, NEWER, ROWS and the keys of BY_NAME as they are; the header declares exactly the entry points; the library builds
with hipcc for gfx950 (no GPU needed), exports exactly them and carries the tree's source id; no other library's source id
sees csrc_pw; scsfm_pw_covers agrees with scsfm_hip.conv1x1's sets; bad arguments are rejected with -1 before any pointer
is touched; the kernels use no scratch, spill nothing and leave room for two workgroups per CU and more; build() reports the
library directly behind opt's line, in its wording."""
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
ENTRY_POINTS = {"scsfm_pw_abi_version", "scsfm_pw_source_id", "scsfm_pw_covers", "scsfm_pw_wrw_ws_bytes",
                "scsfm_pw_wrw_f32", "scsfm_pw_dgrad_f32"}


def test_the_row_is_registered_in_a_fourth_tuple():
    assert [row.name for row in libraries.NEWEST] == ["pw"]
    assert [row.name for row in libraries.NEWER] == ["opt"] and [row.name for row in libraries.LATER] == ["fbn"]
    assert len(libraries.TABLE) == 16
    assert set(libraries.BY_NAME) == {r.name for r in libraries.TABLE} | {"fbn"}
    assert libraries.ROWS == libraries.TABLE + libraries.LATER + libraries.NEWER
    assert libraries.EVERY == libraries.ROWS + libraries.NEWEST
    row = libraries.find("pw")
    assert row is libraries.NEWEST[0] and row.abi == 1 and row.tag == "pw:build" and not row.tag.startswith("build")
    assert all(libraries.find(r.name) is r for r in libraries.EVERY)
    assert row.csrc.endswith("csrc_pw") and row.header.endswith("scsfm_pw.h") and row.lib.endswith("libscsfm_pw.so")
    assert row.prefix == "scsfm_pw_"
    assert "libscsfm_pw.so" in libraries.SUMMARY and "libscsfm_pw.so" in build.__doc__ and "libscsfm_pw.so" in _lib.__doc__
    assert build.PW_LIB == row.lib and build.PW_CSRC == row.csrc and _lib.PW_HEADER == row.header
    assert _lib.PW_LIB_PATH == row.lib and _lib.PW_ABI_VERSION == 1 and callable(_lib.get_pw)
    assert callable(build.build_pw) and callable(build.pw_deps) and callable(build.pw_is_stale)
    assert [os.path.basename(p) for p in build.pw_sources()] == ["scsfm_pointwise.hip"]


def test_other_source_ids_do_not_see_csrc_pw():
    ids = []
    for row in libraries.ROWS:
        deps = build.lib_deps(row.name)
        assert deps and not any("csrc_pw" in p or "scsfm_pw" in p for p in deps), row.name
        ids.append(build.lib_source_id(row.name))
    assert all(os.sep + "csrc_pw" + os.sep in p or p.endswith("scsfm_pw.h") for p in build.pw_deps())
    assert len(set(ids)) == 18 and build.pw_source_id() not in ids


def test_header_declares_exactly_the_entry_points():
    assert set(_lib.parse_header(_lib.PW_HEADER)) == ENTRY_POINTS


def _lib_pw():
    return _lib.CLib(build.build_pw(verbose=False), _lib.PW_HEADER, _lib.PW_ABI_VERSION, "scsfm_pw_")


@needs_hipcc
def test_pw_library_builds_and_exports_its_header():
    path = build.build_pw(verbose=False)
    assert path.endswith("libscsfm_pw.so")
    assert build.binary_source_id(path) == build.pw_source_id() and not build.pw_is_stale()
    lib = _lib_pw()
    assert lib.source_id() == build.pw_source_id()
    assert lib._fn["scsfm_pw_abi_version"]() == 1
    assert set(lib.decls) == ENTRY_POINTS
    nm = shutil.which("nm") or "/opt/rocm/llvm/bin/llvm-nm"
    syms = subprocess.run([nm, "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in syms.splitlines() if " T " in line and "scsfm" in line}
    assert exported == ENTRY_POINTS
    assert _lib.get_pw().path == path


@needs_hipcc
def test_covers_agrees_with_the_python_sets():
    from scsfm_hip import conv1x1 as PW
    lib = _lib_pw()
    channels = (1, 6, 16, 32, 48, 64, 96, 128, 192, 256, 384, 512, 1024, 2048)
    for cin in channels:
        for cout in channels:
            for s in (0, 1, 2, 3, 4):
                assert bool(lib.size("scsfm_pw_covers", cin, cout, s)) == PW.covers(cin, cout, s), (cin, cout, s)
    assert all(PW.covers(*t) for t in PW.ROUTED) and all(PW.dgrad_covers(*t) for t in PW.ROUTED_DGRAD)
    assert PW.ROUTED_DGRAD <= PW.ROUTED


@needs_hipcc
def test_argument_errors_return_minus_one():
    lib = _lib_pw()
    p = ctypes.c_void_p(256)  # never dereferenced: every call below is rejected before anything is launched
    wrw, dgrad, ws_bytes = (lib._fn[n] for n in ("scsfm_pw_wrw_f32", "scsfm_pw_dgrad_f32", "scsfm_pw_wrw_ws_bytes"))
    n = ws_bytes(2, 64, 128, 6, 10, 2)
    assert n == 4 * 2 * 128 * 64
    #       B Cin Cout H W stride x dy dw ws ws_bytes stream
    good = [2, 64, 128, 6, 10, 2, p, p, p, p, n, None]
    for k, bad in ((9, None), (9, ctypes.c_void_p(258)), (9, ctypes.c_void_p(257)), (10, n - 4), (10, 0), (6, None),
                   (7, None), (8, None), (1, 48), (1, 32), (2, 64), (2, 16), (5, 3), (5, 0), (5, -2), (0, 0), (0, -1),
                   (3, 0), (4, 0), (3, -5)):
        args = list(good)
        args[k] = bad
        assert wrw(*args) == -1, (k, bad)
    #        B Cin Cout H W dy w dx stream
    good_d = [2, 64, 128, 6, 10, p, p, p, None]
    for k, bad in ((5, None), (6, None), (7, None), (1, 48), (2, 96), (0, 0), (3, 0), (4, -1)):
        args = list(good_d)
        args[k] = bad
        assert dgrad(*args) == -1, (k, bad)
    # sizes past int: the input, the output gradient, and the pixel count with its tile
    big = 2 ** 31 - 1
    for B, cin, cout, H, W, s in ((1, 64, 128, 65536, 512, 2), (4, 512, 128, 1024, 1024, 1), (big, 64, 128, 1, 1, 2),
                                  (1, 64, 128, big, 2, 2), (1, 64, 128, 2, big, 1), (8192, 64, 512, 512, 1, 1),
                                  (1, 64, 128, 46341, 46341, 1)):
        assert ws_bytes(B, cin, cout, H, W, s) == 0, (B, cin, cout, H, W, s)
        assert wrw(B, cin, cout, H, W, s, p, p, p, p, 1 << 40, None) == -1
        if s == 2:
            assert dgrad(B, cin, cout, H, W, p, p, p, None) == -1
    assert ws_bytes(1, 64, 128, 2048, 4096, 2) == 4 * 512 * 128 * 64  # (2^29 input elements: the largest sizes pass)
    assert lib._fn["scsfm_pw_source_id"](None, 64) == -1


@needs_hipcc
def test_no_kernel_spills_to_scratch(tmp_path):
    """The compiler's resource usage of the three kernels (read as tests/test_opt_library.py reads it): no scratch, no
    spilled register, and registers and LDS for at least two workgroups of four waves per CU -- the stated occupancy is
    waves per SIMD, and a workgroup puts one wave on each of the four; the LDS of a workgroup fits 160 KiB / 2 several
    times over.  The matrix instruction is in both gradient kernels."""
    out = tmp_path / "pw.s"
    flags = [f for f in build.FLAGS if f not in ("-shared", "-fPIC")]
    (src,) = build.pw_sources()
    subprocess.run([HIPCC, *flags, "-S", "--cuda-device-only", "-I", os.path.join(ROOT, "include"), "-o", str(out), src],
                   check=True, capture_output=True)
    text = open(out).read()
    kernels = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M)
    num = lambda key: [int(x) for x in re.findall(r";\s*" + key + r":\s*(\d+)", text)]  # noqa: E731
    scratch, vgprs, lds, occupancy = num("ScratchSize"), num("NumVgprs"), num("LDSByteSize"), num("Occupancy")
    spills = [int(x) for x in re.findall(r"\.[sv]gpr_spill_count:\s*(\d+)", text)]
    assert len(kernels) == 3 and len(scratch) == len(vgprs) == len(lds) == len(occupancy) == 3, (kernels, scratch)
    assert len(spills) == 6, spills
    assert any("wrw_kernel" in k for k in kernels) and any("dgrad_kernel" in k for k in kernels)
    assert scratch == [0, 0, 0] and not any(spills), (scratch, spills)
    assert all(v <= 128 for v in vgprs) and all(o >= 4 for o in occupancy), (vgprs, occupancy)
    assert all(b <= 32 * 1024 for b in lds), lds
    assert text.count("v_mfma_f32_16x16x4_f32 ") == 64 + 32  # (8 pixel steps x 8 blocks, 8 channel steps x 4 blocks)


@needs_hipcc
def test_build_reports_the_library_directly_behind_the_newer_lines(capsys):
    import sys
    sys.path.insert(0, ROOT)
    import __graft_entry__ as G
    G.build()
    out = capsys.readouterr().out.splitlines()
    mine = [i for i, line in enumerate(out) if line.startswith("[pw:build] ")]
    assert len(mine) == 1
    assert out[mine[0]] == f"[pw:build] {build.PW_LIB}: {len(ENTRY_POINTS)} entry points resolved (ABI 1)"
    first = min(i for i, line in enumerate(out) if "entry points resolved" in line)
    assert out[first].startswith("[opt:build] ") and mine[0] == first + len(libraries.NEWER)
    reports = [i for i, line in enumerate(out) if line.endswith("entry points resolved")]
    assert len(reports) == 17 and reports[0] == mine[0] + 1 and out[reports[0]].startswith("[fbn:build] ")
    assert len([line for line in out if line.startswith("[build")]) == 10
    assert out[-2].startswith("[build:vis] ") and out[-1].startswith("[build:prep] ")
