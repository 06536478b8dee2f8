"""libscsfm_dgrad.so: the header parses to exactly its entry points and agrees with what scsfm_hip.decoder_dgrad passes,
the library builds with hipcc for gfx950 (no GPU needed), exports those symbols and nothing else, carries the ABI version
and the tree's source id, leaves the other libraries' source ids alone, agrees with the Python side on what it covers,
rejects bad arguments with -1 before anything is launched, and its kernels use no scratch and stay inside the budget
DESIGN §5xc states (the tail: at most 128 vector registers, four waves per SIMD or more, at most 4 KB of LDS per
workgroup; the data gradient: three workgroups per CU, so at most 53 KB of LDS and 168 vector registers, accumulators
included);
build() reports it under its own tag ahead of the "[build" lines."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

from scsfm_hip import _lib, build, conv_wrw, decoder_dgrad

HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
needs_hipcc = pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc on this machine")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = {"scsfm_dgrad_abi_version", "scsfm_dgrad_source_id", "scsfm_dgrad_head_tail_covers",
                "scsfm_dgrad_head_tail_ws_bytes", "scsfm_dgrad_head_tail_bwd_f32", "scsfm_dgrad_conv3x3_covers",
                "scsfm_dgrad_conv3x3_f32"}
OTHERS = ("", "nets_", "eval_", "odom_", "enc_", "stem_", "snip_", "prep_", "vis_", "dvis_", "val_", "enceval_",
          "decb_", "wrw_", "vlog_")


def test_other_source_ids_do_not_see_csrc_dgrad():
    for prefix in OTHERS:
        deps = getattr(build, prefix + "deps")()
        assert deps and not any("csrc_dgrad" in p or "scsfm_dgrad" in p for p in deps), prefix
    assert build.dgrad_sources() and all(os.sep + "csrc_dgrad" + os.sep in p for p in build.dgrad_sources())
    assert all(os.sep + "csrc_dgrad" + os.sep in p or p.endswith("scsfm_dgrad.h") for p in build.dgrad_deps())
    ids = [getattr(build, prefix + "source_id")() for prefix in OTHERS]
    assert len(set(ids)) == len(OTHERS) and build.dgrad_source_id() not in ids


def test_header_declares_exactly_the_entry_points():
    decls = _lib.parse_header(_lib.DGRAD_HEADER)
    assert set(decls) == ENTRY_POINTS
    ret, args = decls["scsfm_dgrad_head_tail_bwd_f32"]
    assert ret is ctypes.c_int and args == [ctypes.c_int] * 4 + [ctypes.c_float] + [ctypes.c_void_p] * 7 + \
        [ctypes.c_size_t] + [ctypes.c_void_p] * 3
    assert decls["scsfm_dgrad_head_tail_ws_bytes"] == (ctypes.c_size_t, [ctypes.c_int] * 4)
    assert decls["scsfm_dgrad_head_tail_covers"] == (ctypes.c_int, [ctypes.c_int])
    assert decls["scsfm_dgrad_conv3x3_covers"] == (ctypes.c_int, [ctypes.c_int] * 2)
    assert decls["scsfm_dgrad_conv3x3_f32"] == (ctypes.c_int, [ctypes.c_int] * 5 + [ctypes.c_void_p] * 4)


def _lib_dgrad():
    return _lib.CLib(build.build_dgrad(verbose=False), _lib.DGRAD_HEADER, _lib.DGRAD_ABI_VERSION, "scsfm_dgrad_")


@needs_hipcc
def test_dgrad_library_builds_and_exports_its_header():
    path = build.build_dgrad(verbose=False)
    assert path.endswith("libscsfm_dgrad.so")
    assert build.binary_source_id(path) == build.dgrad_source_id() and not build.dgrad_is_stale()
    lib = _lib_dgrad()
    assert lib.source_id() == build.dgrad_source_id()
    assert lib._fn["scsfm_dgrad_abi_version"]() == _lib.DGRAD_ABI_VERSION == 1
    assert set(lib.decls) == ENTRY_POINTS
    nm = shutil.which("nm") or "/opt/rocm/llvm/bin/llvm-nm"
    syms = subprocess.run([nm, "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in syms.splitlines() if " T " in line and "scsfm" in line}
    assert exported == ENTRY_POINTS
    assert _lib.get_dgrad().path == path


@needs_hipcc
def test_coverage_workspace_and_rejected_arguments():
    lib = _lib_dgrad()
    covers = lib._fn["scsfm_dgrad_head_tail_covers"]
    for C in (1, 8, 15, 16, 17, 32, 64):
        assert covers(C) == int(decoder_dgrad.covers(C)) == int(C == 16), C
    size = lambda *a: lib.size("scsfm_dgrad_head_tail_ws_bytes", *a)  # noqa: E731
    # 17 fp64 partials per workgroup, one workgroup per 8 x 64 tile
    assert size(12, 16, 256, 832) == 8 * 17 * 12 * 32 * 13 and size(2, 16, 17, 67) == 8 * 17 * 2 * 3 * 2
    assert size(1, 16, 2, 2) == 8 * 17
    for bad in ((0, 16, 4, 4), (1, 16, 1, 4), (1, 16, 4, 1), (1, 16, 4, -1), (1, 8, 4, 4), (1, 32, 4, 4),
                (1 << 14, 16, 128, 64)):
        assert size(*bad) == 0, bad
    p = ctypes.c_void_p(256)  # never dereferenced: every call below is rejected before anything is launched
    fn = lib._fn["scsfm_dgrad_head_tail_bwd_f32"]
    n = size(2, 16, 5, 67)
    good = [2, 16, 5, 67, 10.0, p, p, p, p, p, p, p, n, p, p, None]
    for k, bad in ((0, 0), (1, 8), (2, 1), (3, 0), (5, None), (7, None), (8, None), (9, None), (10, None), (11, None),
                   (11, ctypes.c_void_p(260)), (12, n - 1), (12, 0)):
        args = list(good)
        args[k] = bad
        assert fn(*args) == -1, (k, bad)
    covers = lib._fn["scsfm_dgrad_conv3x3_covers"]
    for cin in (1, 8, 16, 17, 32, 64, 96):
        for cout in (1, 8, 16, 32):
            assert covers(cin, cout) == int(conv_wrw.dgrad_covers(cin, cout)) == int(cin in (16, 32) and cout == 16)
    assert all(conv_wrw.dgrad_covers(*p) for p in conv_wrw.ROUTED_DGRAD) and conv_wrw.ROUTED_DGRAD <= conv_wrw.ROUTED
    fn = lib._fn["scsfm_dgrad_conv3x3_f32"]
    good = [2, 16, 16, 5, 67, p, p, p, None]
    for k, bad in ((0, 0), (1, 8), (1, 64), (2, 1), (2, 32), (3, 0), (4, 0), (5, None), (6, None), (7, None),
                   (0, 1 << 20)):
        args = list(good)
        args[k] = bad
        assert fn(*args) == -1, (k, bad)


@needs_hipcc
def test_no_kernel_uses_scratch_and_the_budget_holds(tmp_path):
    flags = [f for f in build.FLAGS if f not in ("-shared", "-fPIC")]
    class r:  # (one compilation per source file; their remarks one after the other)
        stderr = "".join(subprocess.run([HIPCC, *flags, "-c", "--cuda-device-only",
                                         "-Rpass-analysis=kernel-resource-usage", "-I", build.INCLUDE, "-o",
                                         str(tmp_path / f"dgrad{k}.o"), src], check=True, capture_output=True,
                                        text=True).stderr for k, src in enumerate(build.dgrad_sources()))
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    vgprs = [int(v) for v in re.findall(r"\bVGPRs: (\d+)", r.stderr)]
    agprs = [int(v) for v in re.findall(r"\bAGPRs: (\d+)", r.stderr)]
    spills = [int(v) for v in re.findall(r"VGPRs Spill: (\d+)", r.stderr)]
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    occupancy = [int(v) for v in re.findall(r"Occupancy \[waves/SIMD\]: (\d+)", r.stderr)]
    lds = [int(v) for v in re.findall(r"LDS Size \[bytes/block\]: (\d+)", r.stderr)]
    # the two instantiations of the tail kernel (with and without the sums), the sum of the partials, and the two
    # instantiations of the data gradient (Cin = 16 and 32)
    assert len(names) == 5, r.stderr[-2000:]
    assert len(vgprs) == len(agprs) == len(scratch) == len(occupancy) == len(spills) == len(lds) == 5, r.stderr[-2000:]
    assert all(s == 0 for s in scratch) and all(s == 0 for s in spills), (names, scratch, spills)
    conv = [k for k, name in enumerate(names) if "conv3x3_dgrad" in name]
    assert len(conv) == 2
    for k in range(5):
        if k in conv:
            assert vgprs[k] + agprs[k] <= 168 and occupancy[k] >= 3 and lds[k] <= 53 * 1024, (names[k], vgprs[k], lds[k])
        else:
            assert vgprs[k] + agprs[k] <= 128 and occupancy[k] >= 4 and lds[k] <= 4096, (names[k], vgprs[k], lds[k])


@needs_hipcc
def test_build_reports_the_library_ahead_of_the_build_lines(capsys):
    import sys
    sys.path.insert(0, ROOT)
    import __graft_entry__ as G
    G.build()
    out = capsys.readouterr().out.splitlines()
    mine = [i for i, line in enumerate(out) if line.startswith("[dgrad:build] ")]
    assert len(mine) == 1
    assert out[mine[0]] == f"[dgrad:build] {build.DGRAD_LIB}: {len(ENTRY_POINTS)} entry points resolved"
    first = min(i for i, line in enumerate(out) if line.startswith("[build"))
    assert mine[0] < first and len([line for line in out if line.startswith("[build")]) == 10
