"""libscsfm_enceval.so: builds with hipcc for gfx950 (no GPU needed), exports exactly the symbols include/scsfm_enceval.h
declares, rejects bad arguments with -1 before touching any pointer, leaves the other eleven libraries' source ids alone,
none of its kernels spills to scratch, and build() reports it under its own tag ahead of the "[build" lines."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

from scsfm_hip import _lib, build

HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
needs_hipcc = pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc on this machine")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = {"scsfm_enceval_abi_version", "scsfm_enceval_source_id", "scsfm_enceval_bn_f32",
                "scsfm_enceval_bn_relu_pool_f32", "scsfm_enceval_maxpool_f32"}
OTHERS = ("", "nets_", "eval_", "odom_", "enc_", "stem_", "snip_", "prep_", "vis_", "dvis_", "val_")


def test_other_source_ids_do_not_see_csrc_enceval():
    for prefix in OTHERS:
        deps = getattr(build, prefix + "deps")()
        assert deps and not any("csrc_enceval" in p or "scsfm_enceval" in p for p in deps), prefix
    assert build.enceval_sources() and all(os.sep + "csrc_enceval" + os.sep in p for p in build.enceval_sources())
    assert all(os.sep + "csrc_enceval" + os.sep in p or p.endswith("scsfm_enceval.h") for p in build.enceval_deps())
    ids = [getattr(build, prefix + "source_id")() for prefix in OTHERS]
    assert len(set(ids)) == 11 and build.enceval_source_id() not in ids


def test_header_declares_exactly_the_entry_points():
    assert set(_lib.parse_header(_lib.ENCEVAL_HEADER)) == ENTRY_POINTS


def _lib_enceval():
    return _lib.CLib(build.build_enceval(verbose=False), _lib.ENCEVAL_HEADER, _lib.ENCEVAL_ABI_VERSION,
                     "scsfm_enceval_")


@needs_hipcc
def test_enceval_library_builds_and_exports_its_header():
    path = build.build_enceval(verbose=False)
    assert path.endswith("libscsfm_enceval.so")
    assert build.binary_source_id(path) == build.enceval_source_id() and not build.enceval_is_stale()
    lib = _lib_enceval()
    assert lib.source_id() == build.enceval_source_id()
    assert lib._fn["scsfm_enceval_abi_version"]() == 1
    assert set(lib.decls) == ENTRY_POINTS
    nm = shutil.which("nm") or "/opt/rocm/llvm/bin/llvm-nm"
    syms = subprocess.run([nm, "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in syms.splitlines() if " T " in line and "scsfm" in line}
    assert exported == ENTRY_POINTS
    assert _lib.get_enceval().path == path


@needs_hipcc
def test_argument_errors_return_minus_one():
    lib = _lib_enceval()
    p = ctypes.c_void_p(256)  # never dereferenced: every call below is rejected before anything is launched
    nan, inf = float("nan"), float("inf")
    fn = lib._fn["scsfm_enceval_bn_f32"]
    #       B  C  H  W  mode eps  x  identity gamma beta rm rv y  stream
    good = [2, 4, 3, 5, 2, 1e-5, p, p, p, p, p, p, p, None]
    for k, bad in ((0, 0), (1, 0), (2, -1), (3, 0), (0, 1 << 30), (4, 3), (4, -1), (5, -1e-5), (5, nan), (5, inf),
                   (5, -inf), (6, None), (7, None), (8, None), (9, None), (10, None), (11, None), (12, None)):
        args = list(good)
        args[k] = bad
        assert fn(*args) == -1, (k, bad)
    assert fn(1 << 15, 1 << 8, 1 << 4, 1 << 4, 1, 1e-5, p, None, p, p, p, p, p, None) == -1  # 2^31 elements
    fn = lib._fn["scsfm_enceval_bn_relu_pool_f32"]
    good = [2, 4, 3, 5, 1e-5, p, p, p, p, p, p, p, None]
    for k, bad in ((0, 0), (1, -2), (2, 0), (3, 0), (1, 1 << 30), (4, -1.0), (4, nan), (4, inf), (5, None), (6, None),
                   (7, None), (8, None), (9, None), (10, None), (11, None)):
        args = list(good)
        args[k] = bad
        assert fn(*args) == -1, (k, bad)
    fn = lib._fn["scsfm_enceval_maxpool_f32"]
    good = [2, 4, 3, 5, p, p, None]
    for k, bad in ((0, 0), (1, 0), (2, 0), (3, -1), (4, None), (5, None), (0, 1 << 30)):
        args = list(good)
        args[k] = bad
        assert fn(*args) == -1, (k, bad)
    assert lib._fn["scsfm_enceval_source_id"](None, 64) == -1


@needs_hipcc
def test_no_kernel_spills_to_scratch(tmp_path):
    """The compiler's resource usage of every kernel of the library (read as tests/test_encoder_library.py reads it): no
    scratch, no LDS, and at most 64 vector registers so that eight waves per SIMD stay resident -- these kernels hide
    memory latency with occupancy."""
    out = tmp_path / "enceval.s"
    flags = [f for f in build.FLAGS if f not in ("-shared", "-fPIC")]
    (src,) = build.enceval_sources()
    subprocess.run([HIPCC, *flags, "-S", "--cuda-device-only", "-I", os.path.join(ROOT, "include"), "-o", str(out), src],
                   check=True, capture_output=True)
    text = open(out).read()
    kernels = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M)
    scratch = [int(x) for x in re.findall(r";\s*ScratchSize:\s*(\d+)", text)]
    vgprs = [int(x) for x in re.findall(r";\s*NumVgprs:\s*(\d+)", text)]
    lds = [int(x) for x in re.findall(r";\s*LDSByteSize:\s*(\d+)", text)]
    # BatchNorm: 2 widths x 3 modes; pool: 2 widths x (fused, plain)
    assert len(kernels) == 10 and len(scratch) == len(kernels) == len(vgprs) == len(lds), (kernels, scratch)
    assert all(s == 0 for s in scratch), dict(zip(kernels, scratch))
    assert all(v <= 64 for v in vgprs), dict(zip(kernels, vgprs))
    assert all(b == 0 for b in lds), dict(zip(kernels, lds))


@needs_hipcc
def test_build_reports_the_library_ahead_of_the_build_lines(capsys):
    import sys
    sys.path.insert(0, ROOT)
    import __graft_entry__ as G
    G.build()
    out = capsys.readouterr().out.splitlines()
    mine = [i for i, line in enumerate(out) if line.startswith("[enceval:build] ")]
    assert len(mine) == 1
    assert out[mine[0]] == f"[enceval:build] {build.ENCEVAL_LIB}: {len(ENTRY_POINTS)} entry points resolved"
    first = min(i for i, line in enumerate(out) if line.startswith("[build"))
    assert mine[0] < first and len([line for line in out if line.startswith("[build")]) == 10
