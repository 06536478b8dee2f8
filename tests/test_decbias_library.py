"""libscsfm_decb.so: builds with hipcc for gfx950 (no GPU needed), exports exactly the symbols include/scsfm_decb.h
declares, carries the ABI version and the tree's source id, leaves the other libraries' source ids alone, none of its
kernels uses scratch, and build() reports it under its own tag ahead of the "[build" lines."""
import os
import re
import shutil
import subprocess

import pytest

from scsfm_hip import _lib, build

HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
needs_hipcc = pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc on this machine")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = {"scsfm_decb_abi_version", "scsfm_decb_source_id", "scsfm_decb_ws_bytes",
                "scsfm_decb_bias_elu_pad_fwd_f32", "scsfm_decb_bias_elu_pad_bwd_f32",
                "scsfm_decb_bias_up_cat_pad_fwd_f32", "scsfm_decb_bias_up_cat_pad_bwd_f32",
                "scsfm_decb_disp_head_fwd_f32", "scsfm_decb_disp_head_bwd_f32"}
OTHERS = ("", "nets_", "eval_", "odom_", "enc_", "stem_", "snip_", "prep_", "vis_", "dvis_", "val_", "enceval_")


def test_other_source_ids_do_not_see_csrc_decb():
    for prefix in OTHERS:
        deps = getattr(build, prefix + "deps")()
        assert deps and not any("csrc_decb" in p or "scsfm_decb" in p for p in deps), prefix
    assert build.decb_sources() and all(os.sep + "csrc_decb" + os.sep in p for p in build.decb_sources())
    assert all(os.sep + "csrc_decb" + os.sep in p or p.endswith("scsfm_decb.h") for p in build.decb_deps())
    ids = [getattr(build, prefix + "source_id")() for prefix in OTHERS]
    assert len(set(ids)) == len(OTHERS) and build.decb_source_id() not in ids


def test_header_declares_exactly_the_entry_points():
    assert set(_lib.parse_header(_lib.DECB_HEADER)) == ENTRY_POINTS


@needs_hipcc
def test_decb_library_builds_and_exports_its_header():
    path = build.build_decb(verbose=False)
    assert path.endswith("libscsfm_decb.so")
    assert build.binary_source_id(path) == build.decb_source_id() and not build.decb_is_stale()
    lib = _lib.CLib(path, _lib.DECB_HEADER, _lib.DECB_ABI_VERSION, "scsfm_decb_")
    assert lib.source_id() == build.decb_source_id()
    assert lib._fn["scsfm_decb_abi_version"]() == _lib.DECB_ABI_VERSION == 1
    assert set(lib.decls) == ENTRY_POINTS
    nm = shutil.which("nm") or "/opt/rocm/llvm/bin/llvm-nm"
    syms = subprocess.run([nm, "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in syms.splitlines() if " T " in line and "scsfm" in line}
    assert exported == ENTRY_POINTS
    assert _lib.get_decb().path == path
    # rejected arguments come back as -1 before anything is launched; the workspace formula of the header
    assert lib._fn["scsfm_decb_bias_elu_pad_fwd_f32"](1, 1, 1, 4, None, None, None, None) == -1
    assert lib._fn["scsfm_decb_disp_head_bwd_f32"](1, 1, 4, 4, 10.0, None, None, None, None, None, None) == -1
    assert lib.size("scsfm_decb_ws_bytes", 12, 16, 256, 832) == 8 * 12 * 16 * 256 * 4
    assert lib.size("scsfm_decb_ws_bytes", 12, 1, 1, 256 * 832) == 8 * 12 * 832


@needs_hipcc
def test_no_kernel_uses_scratch(tmp_path):
    """The compiler's resource usage of every kernel: no scratch (so nothing spills), at most 64 vector registers and
    eight waves per SIMD -- these kernels hide memory latency with occupancy, as libscsfm_nets.so's do."""
    flags = [f for f in build.FLAGS if f not in ("-shared", "-fPIC")]
    r = subprocess.run([HIPCC, *flags, "-c", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-I",
                        build.INCLUDE, "-o", str(tmp_path / "decb.o"), *build.decb_sources()],
                       check=True, capture_output=True, text=True)
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    vgprs = [int(v) for v in re.findall(r"\bVGPRs: (\d+)", r.stderr)]
    spills = [int(v) for v in re.findall(r"VGPRs Spill: (\d+)", r.stderr)]
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    occupancy = [int(v) for v in re.findall(r"Occupancy \[waves/SIMD\]: (\d+)", r.stderr)]
    # two forwards, the head's forward, three backwards with and without the sum, the per-channel sum
    assert len(names) == 10 and len(vgprs) == len(scratch) == len(occupancy) == len(spills) == 10, r.stderr[-2000:]
    assert all(s == 0 for s in scratch) and all(s == 0 for s in spills), (names, scratch, spills)
    assert max(vgprs) <= 64 and min(occupancy) == 8, (names, vgprs, occupancy)


@needs_hipcc
def test_build_reports_the_library_ahead_of_the_build_lines(capsys):
    import sys
    sys.path.insert(0, ROOT)
    import __graft_entry__ as G
    G.build()
    out = capsys.readouterr().out.splitlines()
    mine = [i for i, line in enumerate(out) if line.startswith("[decb:build] ")]
    assert len(mine) == 1
    assert out[mine[0]] == f"[decb:build] {build.DECB_LIB}: {len(ENTRY_POINTS)} entry points resolved"
    first = min(i for i, line in enumerate(out) if line.startswith("[build"))
    assert mine[0] < first and len([line for line in out if line.startswith("[build")]) == 10
