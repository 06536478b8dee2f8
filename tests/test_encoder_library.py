"""libscsfm_enc.so: builds with hipcc for gfx950 (no GPU needed), exports exactly the symbols include/scsfm_enc.h
declares, rejects bad arguments with -1 before touching any pointer, leaves the other four libraries' source ids alone,
and none of its kernels spills to scratch."""
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


def test_other_source_ids_do_not_see_csrc_enc():
    others = build.deps() + build.nets_deps() + build.eval_deps() + build.odom_deps()
    assert not any("csrc_enc" in p or "scsfm_enc" in p for p in others)
    assert build.enc_sources() and all("csrc_enc" in p for p in build.enc_sources())
    assert all(os.sep + "csrc_enc" + os.sep in p or p.endswith("scsfm_enc.h") for p in build.enc_deps())
    ids = (build.source_id(), build.nets_source_id(), build.eval_source_id(), build.odom_source_id())
    assert build.enc_source_id() not in ids and len(set(ids)) == 4


def _lib_enc():
    return _lib.CLib(build.build_enc(verbose=False), _lib.ENC_HEADER, _lib.ENC_ABI_VERSION, "scsfm_enc_")


@needs_hipcc
def test_enc_library_builds_and_exports_its_header():
    path = build.build_enc(verbose=False)
    assert build.binary_source_id(path) == build.enc_source_id() and not build.enc_is_stale()
    lib = _lib_enc()
    assert lib.source_id() == build.enc_source_id()
    assert set(lib.decls) == {"scsfm_enc_abi_version", "scsfm_enc_source_id", "scsfm_enc_bn_workspace_bytes",
                              "scsfm_enc_bn_fwd_f32", "scsfm_enc_bn_bwd_f32", "scsfm_enc_maxpool_fwd_f32",
                              "scsfm_enc_maxpool_bwd_f32"}
    nm = shutil.which("nm") or "/opt/rocm/llvm/bin/llvm-nm"
    syms = subprocess.run([nm, "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in syms.splitlines() if " T " in line and "scsfm" in line}
    assert exported == set(lib.decls)
    assert _lib.get_enc().path == path


@needs_hipcc
def test_argument_errors_return_minus_one():
    lib = _lib_enc()
    p = ctypes.c_void_p(256)  # never dereferenced: every call below is rejected before anything is launched
    assert lib.size("scsfm_enc_bn_workspace_bytes", 12, 64, 128, 416) >= 64 * 2 * 8
    assert lib.size("scsfm_enc_bn_workspace_bytes", 1, 4, 1, 1) == 0  # one entry per channel: no variance
    assert lib.size("scsfm_enc_bn_workspace_bytes", 0, 4, 2, 2) == 0
    assert lib.size("scsfm_enc_bn_workspace_bytes", 64, 1024, 256, 256) == 0  # 2^32 elements
    n = lib.size("scsfm_enc_bn_workspace_bytes", 2, 4, 3, 5)
    fn = lib._fn["scsfm_enc_bn_fwd_f32"]
    good = [2, 4, 3, 5, 2, 1e-5, 0.1, p, p, p, p, p, p, p, p, p, p, n, None]
    for k, bad in ((0, 0), (1, 0), (2, -1), (3, 0), (4, 3), (4, -1), (5, -1.0), (6, 1.5), (6, float("nan")), (7, None),
                   (8, None), (9, None), (10, None), (11, None), (12, None), (13, None), (14, None), (15, None),
                   (16, None), (16, ctypes.c_void_p(260)), (17, n - 1)):
        args = list(good)
        args[k] = bad
        assert fn(*args) == -1, (k, bad)
    assert fn(1, 4, 1, 1, 1, 1e-5, 0.1, p, p, p, p, p, p, p, p, p, p, 1 << 20, None) == -1
    fn = lib._fn["scsfm_enc_bn_bwd_f32"]
    good = [2, 4, 3, 5, 2, p, p, p, p, p, p, p, p, p, p, p, n, None]
    for k, bad in ((0, 0), (1, -3), (2, 0), (3, 0), (4, 3), (5, None), (6, None), (7, None), (8, None), (9, None),
                   (10, None), (11, None), (12, None), (13, None), (14, None), (15, None), (16, n - 1)):
        args = list(good)
        args[k] = bad
        assert fn(*args) == -1, (k, bad)
    for name in ("scsfm_enc_maxpool_fwd_f32", "scsfm_enc_maxpool_bwd_f32"):
        fn = lib._fn[name]
        good = [2, 4, 3, 5, p, p, p, None]
        for k, bad in ((0, 0), (1, 0), (2, 0), (3, -1), (4, None), (5, None), (6, None), (0, 1 << 30)):
            args = list(good)
            args[k] = bad
            assert fn(*args) == -1, (name, k, bad)


@needs_hipcc
def test_no_kernel_spills_to_scratch(tmp_path):
    """The compiler's resource usage of every kernel of the library (read as tests/test_odom_library.py reads it): no
    scratch, and at most 64 vector registers so that eight waves per SIMD stay resident -- these kernels hide memory
    latency with occupancy."""
    out = tmp_path / "enc.s"
    flags = [f for f in build.FLAGS if f not in ("-shared", "-fPIC")]
    for src in build.enc_sources():
        subprocess.run([HIPCC, *flags, "-S", "--cuda-device-only", "-I", os.path.join(ROOT, "include"), "-o", str(out),
                        src], check=True, capture_output=True)
        text = open(out).read()
        kernels = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M)
        scratch = [int(x) for x in re.findall(r";\s*ScratchSize:\s*(\d+)", text)]
        vgprs = [int(x) for x in re.findall(r";\s*NumVgprs:\s*(\d+)", text)]
        assert len(kernels) == 22 and len(scratch) == len(kernels) == len(vgprs), (kernels, scratch)
        assert all(s == 0 for s in scratch), dict(zip(kernels, scratch))
        assert all(v <= 64 for v in vgprs), dict(zip(kernels, vgprs))
