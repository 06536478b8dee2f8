"""libscsfm_dvis.so: builds with hipcc for gfx950 (no GPU needed), exports exactly the symbols include/scsfm_dvis.h
declares with ABI version 1, rejects every documented bad argument with -1 before touching any pointer, leaves the
other nine libraries' source ids alone, and none of its kernels spills to scratch."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from scsfm_hip import _lib, build, depth_vis

HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
needs_hipcc = pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc on this machine")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = {"scsfm_dvis_abi_version", "scsfm_dvis_source_id", "scsfm_dvis_scaled_depth",
                "scsfm_dvis_range_workspace_bytes", "scsfm_dvis_range", "scsfm_dvis_colourise"}


def test_header_and_loader_agree():
    decls = _lib.parse_header(_lib.DVIS_HEADER)
    assert set(decls) == ENTRY_POINTS
    assert decls["scsfm_dvis_range_workspace_bytes"] == (ctypes.c_size_t, [ctypes.c_size_t, ctypes.c_int])
    assert len(decls["scsfm_dvis_scaled_depth"][1]) == 13 and len(decls["scsfm_dvis_range"][1]) == 14
    assert len(decls["scsfm_dvis_colourise"][1]) == 13
    assert _lib.DVIS_ABI_VERSION == 1 and _lib.DVIS_LIB_PATH == build.DVIS_LIB


def test_other_source_ids_do_not_see_csrc_dvis():
    others = build.deps() + build.nets_deps() + build.eval_deps() + build.odom_deps() + build.enc_deps() + \
        build.stem_deps() + build.snip_deps() + build.prep_deps() + build.vis_deps()
    assert not any("csrc_dvis" in p or "scsfm_dvis" in p for p in others)
    assert build.dvis_sources() and all(os.sep + "csrc_dvis" + os.sep in p for p in build.dvis_sources())
    assert all(os.sep + "csrc_dvis" + os.sep in p or p.endswith("scsfm_dvis.h") for p in build.dvis_deps())
    ids = (build.source_id(), build.nets_source_id(), build.eval_source_id(), build.odom_source_id(),
           build.enc_source_id(), build.stem_source_id(), build.snip_source_id(), build.prep_source_id(),
           build.vis_source_id())
    assert build.dvis_source_id() not in ids and len(set(ids)) == 9


def _lib_dvis():
    return _lib.CLib(build.build_dvis(verbose=False), _lib.DVIS_HEADER, _lib.DVIS_ABI_VERSION, "scsfm_dvis_")


@needs_hipcc
def test_dvis_library_builds_and_exports_its_header():
    path = build.build_dvis(verbose=False)
    assert build.binary_source_id(path) == build.dvis_source_id() and not build.dvis_is_stale()
    lib = _lib_dvis()
    assert lib.source_id() == build.dvis_source_id()
    assert lib._fn["scsfm_dvis_abi_version"]() == 1
    assert set(lib.decls) == ENTRY_POINTS
    nm = shutil.which("nm") or "/opt/rocm/llvm/bin/llvm-nm"
    syms = subprocess.run([nm, "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in syms.splitlines() if " T " in line and "scsfm" in line}
    assert exported == ENTRY_POINTS
    assert _lib.get_dvis().path == path


@needs_hipcc
def test_build_reports_the_tenth_library_first(capsys):
    import sys
    sys.path.insert(0, ROOT)
    import __graft_entry__ as G
    G.build()
    out = [line for line in capsys.readouterr().out.splitlines() if line.startswith("[build")]
    assert out[0] == f"[build:dvis] {build.DVIS_LIB}: 6 entry points resolved"
    assert len(out) == 10 and sum(line.startswith("[build:dvis] ") for line in out) == 1


@needs_hipcc
def test_argument_errors_return_minus_one():
    lib = _lib_dvis()
    p = ctypes.c_void_p(256)  # never dereferenced: every call below is rejected before anything is launched
    odd = ctypes.c_void_p(258)
    fn = lib._fn["scsfm_dvis_scaled_depth"]
    #       N  h  w  p64 pred o64 ratio off gh gw max_hw out stream
    good = [2, 5, 7, 0, p, 0, p, p, p, p, 1025, p, None]  # (two blocks per image: 2^30 images overflow the grid)
    for k, bad in ((0, 0), (0, -1), (1, 0), (2, 0), (1, 1 << 30), (3, 2), (3, -1), (3, 1), (5, 2), (4, None), (4, odd),
                   (6, None), (6, odd), (7, None), (7, odd), (8, None), (8, odd), (9, None), (9, odd), (10, 0),
                   (10, -5), (11, None), (11, odd), (0, 1 << 30)):
        args = list(good)
        args[k] = bad
        assert fn(*args) == -1, (k, bad)

    assert lib.size("scsfm_dvis_range_workspace_bytes", 0, 0) == 0
    assert lib.size("scsfm_dvis_range_workspace_bytes", 1 << 40, 0) == 0
    assert lib.size("scsfm_dvis_range_workspace_bytes", 10, 2) == 0
    assert lib.size("scsfm_dvis_range_workspace_bytes", 10, 0) == 256
    assert lib.size("scsfm_dvis_range_workspace_bytes", 65, 1) == 768
    fn = lib._fn["scsfm_dvis_range"]
    #       N  f64 maps off gh gw total lo hi t  ws ws_bytes range stream
    good = [3, 1, p, p, p, p, 100, p, p, p, p, 1024, p, None]
    for k, bad in ((0, 0), (0, -2), (1, 2), (1, -1), (2, None), (2, odd), (3, None), (3, odd), (4, None), (4, odd),
                   (5, None), (5, odd), (6, 0), (6, 1 << 40), (7, None), (7, odd), (8, None), (8, odd), (9, None),
                   (9, odd), (10, None), (10, odd), (11, 1023), (11, 0), (12, None), (12, odd)):
        args = list(good)
        args[k] = bad
        assert fn(*args) == -1, (k, bad)

    fn = lib._fn["scsfm_dvis_colourise"]
    #       N  f64 maps off gh gw max_hw range table out out_off pitch stream
    good = [3, 0, p, p, p, p, 1025, p, p, p, p, p, None]
    for k, bad in ((0, 0), (1, 2), (2, None), (2, odd), (3, None), (3, odd), (4, None), (4, odd), (5, None), (5, odd),
                   (6, 0), (6, -1), (7, None), (7, odd), (8, None), (9, None), (10, None), (10, odd), (11, None),
                   (11, odd), (0, 1 << 30)):
        args = list(good)
        args[k] = bad
        assert fn(*args) == -1, (k, bad)
    assert lib._fn["scsfm_dvis_source_id"](None, 64) == -1


@needs_hipcc
def test_no_kernel_spills_to_scratch(tmp_path):
    """The compiler's resource usage of every kernel of the library (read as tests/test_vis_library.py reads it)."""
    out = tmp_path / "dvis.s"
    flags = [f for f in build.FLAGS if f not in ("-shared", "-fPIC")]
    n = 0
    for src in build.dvis_sources():
        subprocess.run([HIPCC, *flags, "-S", "--cuda-device-only", "-I", os.path.join(ROOT, "include"), "-o", str(out),
                        src], check=True, capture_output=True)
        text = open(out).read()
        kernels = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M)
        scratch = [int(x) for x in re.findall(r";\s*ScratchSize:\s*(\d+)", text)]
        vgprs = [int(x) for x in re.findall(r";\s*NumVgprs:\s*(\d+)", text)]
        assert len(scratch) == len(kernels) == len(vgprs), (kernels, scratch)
        assert all(s == 0 for s in scratch), dict(zip(kernels, scratch))
        assert all(v <= 128 for v in vgprs), dict(zip(kernels, vgprs))  # (the range kernel runs 1024 lanes)
        # every division is the full one, in both precisions (no bare reciprocal multiply)
        assert "v_div_fixup_f32" in text and "v_div_fixup_f64" in text
        n += len(kernels)
    # scaled (3 precisions), range (2), colourise (2)
    assert n == 7


def test_magma_table_and_percentile_index():
    assert depth_vis.MAGMA.shape == (256, 3) and depth_vis.MAGMA.dtype == np.uint8
    assert not depth_vis.MAGMA.flags.writeable
    assert depth_vis.MAGMA[0].tolist() == [0, 0, 3] and depth_vis.MAGMA[255].tolist() == [251, 252, 191]
    assert depth_vis.percentile_index(1, np.float32) == (0, 0, 0)
    lo, hi, t = depth_vis.percentile_index(20, np.float64)
    assert (lo, hi) == (18, 19) and isinstance(t, np.float64)
    # 2 207 542 is the smallest n at which the two precisions pick different order statistics
    assert depth_vis.percentile_index(2207542, np.float32)[0] != depth_vis.percentile_index(2207542, np.float64)[0]
    assert all(depth_vis.percentile_index(n, np.float32)[0] == depth_vis.percentile_index(n, np.float64)[0]
               for n in (2, 21, 41, 466650, 2207541))


def test_wrappers_refuse_host_tensors():
    import torch
    with pytest.raises(RuntimeError):
        depth_vis.depth_range([torch.ones(4, 4)])
    with pytest.raises(RuntimeError):
        depth_vis.scaled_depths(torch.ones(1, 4, 4), [1.0], [(4, 4)])
    with pytest.raises(RuntimeError):
        depth_vis.depth_pictures(torch.ones(1, 4, 4))
    with pytest.raises(ValueError):
        depth_vis.depth_range([])
