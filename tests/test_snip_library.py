"""libscsfm_snip.so: builds with hipcc for gfx950 (no GPU needed), exports exactly the symbols include/scsfm_snip.h
declares, rejects bad arguments with -1 before touching any pointer, leaves the other six libraries' source ids alone,
and none of its kernels spills to scratch or needs more than 128 vector registers."""
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


def test_other_source_ids_do_not_see_csrc_snip():
    others = build.deps() + build.nets_deps() + build.eval_deps() + build.odom_deps() + build.enc_deps() + \
        build.stem_deps()
    assert not any("csrc_snip" in p or "scsfm_snip" in p for p in others)
    assert build.snip_sources() and all(os.sep + "csrc_snip" + os.sep in p for p in build.snip_sources())
    assert all(os.sep + "csrc_snip" + os.sep in p or p.endswith("scsfm_snip.h") for p in build.snip_deps())
    ids = (build.source_id(), build.nets_source_id(), build.eval_source_id(), build.odom_source_id(),
           build.enc_source_id(), build.stem_source_id())
    assert build.snip_source_id() not in ids and len(set(ids)) == 6


def _lib_snip():
    return _lib.CLib(build.build_snip(verbose=False), _lib.SNIP_HEADER, _lib.SNIP_ABI_VERSION, "scsfm_snip_")


@needs_hipcc
def test_snip_library_builds_and_exports_its_header():
    path = build.build_snip(verbose=False)
    assert build.binary_source_id(path) == build.snip_source_id() and not build.snip_is_stale()
    lib = _lib_snip()
    assert lib.source_id() == build.snip_source_id()
    assert set(lib.decls) == {"scsfm_snip_abi_version", "scsfm_snip_source_id", "scsfm_snip_workspace_bytes",
                              "scsfm_snip_eval"}
    nm = shutil.which("nm") or "/opt/rocm/llvm/bin/llvm-nm"
    syms = subprocess.run([nm, "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in syms.splitlines() if " T " in line and "scsfm" in line}
    assert exported == set(lib.decls)
    assert _lib.get_snip().path == path


@needs_hipcc
def test_argument_errors_return_minus_one():
    lib = _lib_snip()
    p = ctypes.c_void_p(256)  # never dereferenced: every call below is rejected before anything is launched
    assert lib.size("scsfm_snip_workspace_bytes", 2, 5, 2000) >= 2000 * 96
    for bad in ((0, 5, 2000), (-1, 5, 2000), (2, 1, 2000), (2, 17, 2000), (2, 5, 0), (2, 5, 1 << 30)):
        assert lib.size("scsfm_snip_workspace_bytes", *bad) == 0, bad
    nbytes = lib.size("scsfm_snip_workspace_bytes", 2, 5, 2000)
    fn = lib._fn["scsfm_snip_eval"]
    #       S  L  f64 rot vec gt off len snip total n_snip pred gt_comp errors stats ws  bytes  stream
    good = [2, 5, 0, 0, p, p, p, p, p, 2000, 1992, p, p, p, p, p, nbytes, None]
    for k, bad in ((0, 0), (1, 1), (1, 17), (3, 2), (3, -1), (4, None), (5, None), (6, None), (7, None), (8, None),
                   (9, 0), (10, 0), (10, 2001), (11, None), (13, None), (14, None), (15, None), (16, nbytes - 1)):
        args = list(good)
        args[k] = bad
        assert fn(*args) == -1, (k, bad)
    # (argument 12, gt_comp, may be NULL; that call would launch, so it is made on the simulator and on the GPU)


@needs_hipcc
def test_no_kernel_spills_to_scratch(tmp_path):
    """The compiler's resource usage of every kernel of the library (read as tests/test_odom_library.py reads it): no
    scratch, and at most 128 vector registers so that four waves per SIMD stay resident."""
    out = tmp_path / "snip.s"
    flags = [f for f in build.FLAGS if f not in ("-shared", "-fPIC")]
    for src in build.snip_sources():
        subprocess.run([HIPCC, *flags, "-S", "--cuda-device-only", "-I", os.path.join(ROOT, "include"), "-o", str(out),
                        src], check=True, capture_output=True)
        text = open(out).read()
        kernels = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M)
        scratch = [int(x) for x in re.findall(r";\s*ScratchSize:\s*(\d+)", text)]
        vgprs = [int(x) for x in re.findall(r";\s*NumVgprs:\s*(\d+)", text)]
        # invert x 2 input precisions, snippet, stats
        assert len(kernels) == 4 and len(scratch) == len(kernels) == len(vgprs), (kernels, scratch)
        assert all(s == 0 for s in scratch), dict(zip(kernels, scratch))
        assert all(v <= 128 for v in vgprs), dict(zip(kernels, vgprs))
