"""libscsfm_prep.so: builds with hipcc for gfx950 (no GPU needed), exports exactly the symbols include/scsfm_prep.h
declares, rejects bad arguments with -1 before touching any pointer, leaves the other seven libraries' source ids alone,
and none of its kernels spills to scratch."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import pytest

from scsfm_hip import _lib, build

HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
needs_hipcc = pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc on this machine")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_other_source_ids_do_not_see_csrc_prep():
    others = build.deps() + build.nets_deps() + build.eval_deps() + build.odom_deps() + build.enc_deps() + \
        build.stem_deps() + build.snip_deps()
    assert not any("csrc_prep" in p or "scsfm_prep" in p for p in others)
    assert build.prep_sources() and all(os.sep + "csrc_prep" + os.sep in p for p in build.prep_sources())
    assert all(os.sep + "csrc_prep" + os.sep in p or p.endswith("scsfm_prep.h") for p in build.prep_deps())
    ids = (build.source_id(), build.nets_source_id(), build.eval_source_id(), build.odom_source_id(),
           build.enc_source_id(), build.stem_source_id(), build.snip_source_id())
    assert build.prep_source_id() not in ids and len(set(ids)) == 7


def _lib_prep():
    return _lib.CLib(build.build_prep(verbose=False), _lib.PREP_HEADER, _lib.PREP_ABI_VERSION, "scsfm_prep_")


@needs_hipcc
def test_prep_library_builds_and_exports_its_header():
    path = build.build_prep(verbose=False)
    assert build.binary_source_id(path) == build.prep_source_id() and not build.prep_is_stale()
    lib = _lib_prep()
    assert lib.source_id() == build.prep_source_id()
    assert lib._fn["scsfm_prep_abi_version"]() == _lib.PREP_ABI_VERSION == 1
    assert set(lib.decls) == {"scsfm_prep_abi_version", "scsfm_prep_source_id", "scsfm_prep_resize_workspace_bytes",
                              "scsfm_prep_resize_u8", "scsfm_prep_velo_workspace_bytes", "scsfm_prep_velo_depth"}
    nm = shutil.which("nm") or "/opt/rocm/llvm/bin/llvm-nm"
    syms = subprocess.run([nm, "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in syms.splitlines() if " T " in line and "scsfm" in line}
    assert exported == set(lib.decls)
    assert _lib.get_prep().path == path


@needs_hipcc
def test_build_resolves_the_eighth_library_under_its_own_tag(capsys):
    """build() reports libscsfm_prep.so after the seven "[build] " lines, which stay exactly as they were."""
    sys.path.insert(0, ROOT)
    import __graft_entry__ as G
    G.build()
    out = capsys.readouterr().out.splitlines()
    assert [line.split("/")[-1].split(":")[0] for line in out if line.startswith("[build] ")] == [
        "libscsfm_hip.so", "libscsfm_nets.so", "libscsfm_eval.so", "libscsfm_odom.so", "libscsfm_enc.so",
        "libscsfm_stem.so", "libscsfm_snip.so"]
    mine = [line.split("/")[-1] for line in out if line.startswith("[build:prep] ")]
    assert mine == [f"libscsfm_prep.so: {len(_lib.parse_header(_lib.PREP_HEADER))} entry points resolved"]
    assert mine[0].startswith("libscsfm_prep.so: 6 ") and out[-1] == f"[build:prep] {build.PREP_LIB}: 6 entry points resolved"


@needs_hipcc
def test_workspace_queries():
    lib = _lib_prep()
    assert lib.size("scsfm_prep_resize_workspace_bytes", 4, 3, 416, 375, 1) >= 4 * 3 * 416 * 375
    assert lib.size("scsfm_prep_resize_workspace_bytes", 4, 3, 416, 375, 0) == 0  # one pass: no intermediate
    for bad in ((0, 3, 416, 375, 1), (4, 2, 416, 375, 1), (4, 5, 416, 375, 1), (4, 3, 0, 375, 1), (4, 3, 416, 0, 1),
                (1 << 20, 3, 416, 375, 1)):
        assert lib.size("scsfm_prep_resize_workspace_bytes", *bad) == 0, bad
    assert lib.size("scsfm_prep_velo_workspace_bytes", 2, 128, 416) >= 2 * 4 * (128 * 416 + 3 * (128 * 415 + 1))
    for bad in ((0, 128, 416), (2, 0, 416), (2, 128, 0), (-1, 128, 416), (1 << 12, 1 << 10, 1 << 10)):
        assert lib.size("scsfm_prep_velo_workspace_bytes", *bad) == 0, bad


@needs_hipcc
def test_argument_errors_return_minus_one():
    lib = _lib_prep()
    p = ctypes.c_void_p(256)  # never dereferenced: every call below is rejected before anything is launched
    fn = lib._fn["scsfm_prep_resize_u8"]
    nbytes = lib.size("scsfm_prep_resize_workspace_bytes", 2, 3, 20, 23, 1)
    #       N  H   W   C  keep w   in hrows htaps n  vrows vtaps n  row0 rows out ws  bytes  stream
    good = [2, 23, 61, 3, 8, 20, p, p, p, 140, p, p, 56, 0, 23, p, p, nbytes, None]
    for k, bad in ((0, 0), (1, 0), (2, 0), (3, 2), (3, 5), (4, 0), (5, 0), (6, None), (8, None), (9, 0), (11, None),
                   (12, 0), (13, -1), (13, 1), (14, 0), (14, 24), (15, None), (16, None), (17, nbytes - 1)):
        args = list(good)
        args[k] = bad
        assert fn(*args) == -1, (k, bad)
    skipped = list(good)
    skipped[7] = None  # no horizontal table, but the width changes
    assert fn(*skipped) == -1
    skipped = list(good)
    skipped[10], skipped[4] = None, 24  # no vertical table, but more rows are asked for than the source has
    assert fn(*skipped) == -1

    fn = lib._fn["scsfm_prep_velo_depth"]
    nbytes = lib.size("scsfm_prep_velo_workspace_bytes", 2, 16, 48)
    #       F  h   w   bu    bv    points total off P depth ws bytes stream
    good = [2, 16, 48, 48.0, 16.0, p, 1000, p, p, p, p, nbytes, None]
    for k, bad in ((0, 0), (1, 0), (2, 0), (3, 48.5), (3, 0.0), (3, float("nan")), (4, 16.5), (4, -1.0), (5, None),
                   (6, 1 << 31), (7, None), (8, None), (9, None), (10, None), (11, nbytes - 1)):
        args = list(good)
        args[k] = bad
        assert fn(*args) == -1, (k, bad)


@needs_hipcc
def test_no_kernel_spills_to_scratch(tmp_path):
    """The compiler's resource usage of every kernel of the library (read as tests/test_snip_library.py reads it)."""
    out = tmp_path / "prep.s"
    flags = [f for f in build.FLAGS if f not in ("-shared", "-fPIC")]
    n = 0
    for src in build.prep_sources():
        subprocess.run([HIPCC, *flags, "-S", "--cuda-device-only", "-I", os.path.join(ROOT, "include"), "-o", str(out),
                        src], check=True, capture_output=True)
        text = open(out).read()
        kernels = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M)
        scratch = [int(x) for x in re.findall(r";\s*ScratchSize:\s*(\d+)", text)]
        vgprs = [int(x) for x in re.findall(r";\s*NumVgprs:\s*(\d+)", text)]
        assert len(scratch) == len(kernels) == len(vgprs), (kernels, scratch)
        assert all(s == 0 for s in scratch), dict(zip(kernels, scratch))
        assert all(v <= 128 for v in vgprs), dict(zip(kernels, vgprs))
        n += len(kernels)
    # horizontal pass, vertical pass, copy; clear, collect, resolve
    assert n == 6
