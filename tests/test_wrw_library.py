"""libscsfm_wrw.so: the header parses to exactly its entry points, the library builds with hipcc for gfx950 (no GPU
needed), exports those symbols and nothing else, carries the ABI version and the tree's source id, leaves the other
libraries' source ids alone, rejects bad arguments with -1 before anything is launched, and its kernels use no scratch
and stay inside the registers and the LDS that two workgroups per CU leave each; build() reports it under its own tag
ahead of the "[build" lines."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

from scsfm_hip import _lib, build, conv_wrw

HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
needs_hipcc = pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc on this machine")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = {"scsfm_wrw_abi_version", "scsfm_wrw_source_id", "scsfm_wrw_conv3x3_covers",
                "scsfm_wrw_conv3x3_ws_bytes", "scsfm_wrw_conv3x3_f32"}
OTHERS = ("", "nets_", "eval_", "odom_", "enc_", "stem_", "snip_", "prep_", "vis_", "dvis_", "val_", "enceval_",
          "decb_")


def test_other_source_ids_do_not_see_csrc_wrw():
    for prefix in OTHERS:
        deps = getattr(build, prefix + "deps")()
        assert deps and not any("csrc_wrw" in p or "scsfm_wrw" in p for p in deps), prefix
    assert build.wrw_sources() and all(os.sep + "csrc_wrw" + os.sep in p for p in build.wrw_sources())
    assert all(os.sep + "csrc_wrw" + os.sep in p or p.endswith("scsfm_wrw.h") for p in build.wrw_deps())
    ids = [getattr(build, prefix + "source_id")() for prefix in OTHERS]
    assert len(set(ids)) == len(OTHERS) and build.wrw_source_id() not in ids


def test_header_declares_exactly_the_entry_points():
    decls = _lib.parse_header(_lib.WRW_HEADER)
    assert set(decls) == ENTRY_POINTS
    ret, args = decls["scsfm_wrw_conv3x3_f32"]
    assert ret is ctypes.c_int and args == [ctypes.c_int] * 5 + [ctypes.c_void_p] * 4 + [ctypes.c_size_t,
                                                                                         ctypes.c_void_p]
    assert decls["scsfm_wrw_conv3x3_ws_bytes"] == (ctypes.c_size_t, [ctypes.c_int] * 5)


def _lib_wrw():
    return _lib.CLib(build.build_wrw(verbose=False), _lib.WRW_HEADER, _lib.WRW_ABI_VERSION, "scsfm_wrw_")


@needs_hipcc
def test_wrw_library_builds_and_exports_its_header():
    path = build.build_wrw(verbose=False)
    assert path.endswith("libscsfm_wrw.so")
    assert build.binary_source_id(path) == build.wrw_source_id() and not build.wrw_is_stale()
    lib = _lib_wrw()
    assert lib.source_id() == build.wrw_source_id()
    assert lib._fn["scsfm_wrw_abi_version"]() == _lib.WRW_ABI_VERSION == 1
    assert set(lib.decls) == ENTRY_POINTS
    nm = shutil.which("nm") or "/opt/rocm/llvm/bin/llvm-nm"
    syms = subprocess.run([nm, "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in syms.splitlines() if " T " in line and "scsfm" in line}
    assert exported == ENTRY_POINTS
    assert _lib.get_wrw().path == path


@needs_hipcc
def test_coverage_workspace_and_rejected_arguments():
    lib = _lib_wrw()
    covers = lib._fn["scsfm_wrw_conv3x3_covers"]
    for cin in (1, 8, 16, 17, 32, 48, 64, 96, 128, 256):
        for cout in (1, 8, 16, 32, 64):
            assert covers(cin, cout) == int(conv_wrw.covers(cin, cout)) == int(cin in (16, 32, 64, 96) and
                                                                              cout in (1, 16, 32)), (cin, cout)
    assert conv_wrw.ROUTED <= {(ci, co) for ci in conv_wrw.CIN for co in conv_wrw.COUT}
    size = lambda *a: lib.size("scsfm_wrw_conv3x3_ws_bytes", *a)  # noqa: E731
    # one fp32 partial dW per workgroup: 512 workgroups over the chunks of 32 input channels, at most one per 8 x 32
    # tile
    assert size(12, 96, 32, 128, 416) == 4 * (512 // 3) * 32 * 96 * 9
    assert size(12, 64, 32, 64, 208) == 4 * 256 * 32 * 64 * 9
    assert size(12, 32, 16, 128, 416) == 4 * 512 * 16 * 32 * 9
    assert size(12, 16, 16, 256, 832) == 4 * 512 * 16 * 16 * 9 and size(12, 16, 1, 256, 832) == 4 * 512 * 16 * 9
    assert size(1, 16, 16, 1, 1) == 4 * 16 * 16 * 9 and size(2, 16, 16, 5, 67) == 4 * 6 * 16 * 16 * 9
    for bad in ((0, 16, 16, 4, 4), (1, 16, 16, 0, 4), (1, 16, 16, 4, -1), (1, 24, 16, 4, 4), (1, 16, 64, 4, 4),
                (1, 32, 16, 1 << 14, 1 << 14)):
        assert size(*bad) == 0, bad
    p = ctypes.c_void_p(256)  # never dereferenced: every call below is rejected before anything is launched
    fn = lib._fn["scsfm_wrw_conv3x3_f32"]
    n = size(2, 16, 16, 5, 67)
    good = [2, 16, 16, 5, 67, p, p, p, p, n, None]
    for k, bad in ((0, 0), (1, 8), (2, 2), (3, 0), (4, 0), (5, None), (6, None), (7, None), (8, None),
                   (8, ctypes.c_void_p(258)), (9, n - 1), (9, 0)):
        args = list(good)
        args[k] = bad
        assert fn(*args) == -1, (k, bad)


@needs_hipcc
def test_no_kernel_uses_scratch_and_two_workgroups_fit_a_cu(tmp_path):
    """The compiler's resource usage of every kernel: no scratch and no spill; workgroups of four waves, two of them
    per CU, put two waves on every SIMD, which leaves each 256 of the 512 vector registers (accumulators included) and
    80 KB of the CU's 160 KB of LDS."""
    flags = [f for f in build.FLAGS if f not in ("-shared", "-fPIC")]
    r = subprocess.run([HIPCC, *flags, "-c", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-I",
                        build.INCLUDE, "-o", str(tmp_path / "wrw.o"), *build.wrw_sources()],
                       check=True, capture_output=True, text=True)
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    vgprs = [int(v) for v in re.findall(r"\bVGPRs: (\d+)", r.stderr)]
    agprs = [int(v) for v in re.findall(r"\bAGPRs: (\d+)", r.stderr)]
    spills = [int(v) for v in re.findall(r"VGPRs Spill: (\d+)", r.stderr)]
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    occupancy = [int(v) for v in re.findall(r"Occupancy \[waves/SIMD\]: (\d+)", r.stderr)]
    lds = [int(v) for v in re.findall(r"LDS Size \[bytes/block\]: (\d+)", r.stderr)]
    # the four (Cout, chunk) instantiations of the convolution kernel and the sum of the partials
    assert len(names) == 5, r.stderr[-2000:]
    assert len(vgprs) == len(agprs) == len(scratch) == len(occupancy) == len(spills) == len(lds) == 5, r.stderr[-2000:]
    assert all(s == 0 for s in scratch) and all(s == 0 for s in spills), (names, scratch, spills)
    assert all(v + a <= 256 for v, a in zip(vgprs, agprs)) and min(occupancy) >= 2, (names, vgprs, agprs, occupancy)
    assert max(lds) <= 80 * 1024, (names, lds)


@needs_hipcc
def test_build_reports_the_library_ahead_of_the_build_lines(capsys):
    import sys
    sys.path.insert(0, ROOT)
    import __graft_entry__ as G
    G.build()
    out = capsys.readouterr().out.splitlines()
    mine = [i for i, line in enumerate(out) if line.startswith("[wrw:build] ")]
    assert len(mine) == 1
    assert out[mine[0]] == f"[wrw:build] {build.WRW_LIB}: {len(ENTRY_POINTS)} entry points resolved"
    first = min(i for i, line in enumerate(out) if line.startswith("[build"))
    assert mine[0] < first and len([line for line in out if line.startswith("[build")]) == 10
