"""libscsfm_opt.so, the eighteenth library (scsfm_hip.libraries.NEWER): the row stands in a third tuple and leaves TABLE,
LATER and the keys of BY_NAME as they are; the header declares exactly the entry points; the library builds with hipcc for
gfx950 (no GPU needed) and exports exactly them; bad arguments are rejected with -1 before any pointer is touched; the
kernel uses no scratch, no LDS and at most 64 vector registers; build() reports the library under its own tag ahead of every
other line, in a wording that leaves the counts other tests pin alone."""
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
ENTRY_POINTS = {"scsfm_opt_abi_version", "scsfm_opt_source_id", "scsfm_opt_adam_step_f32"}


def test_the_row_is_registered_in_a_third_tuple():
    assert [row.name for row in libraries.NEWER] == ["opt"]
    assert [row.name for row in libraries.LATER] == ["fbn"] and len(libraries.TABLE) == 16
    assert set(libraries.BY_NAME) == {r.name for r in libraries.TABLE} | {"fbn"}
    assert libraries.ROWS == libraries.TABLE + libraries.LATER + libraries.NEWER
    row = libraries.find("opt")
    assert row is libraries.NEWER[0] and row.abi == 1 and row.tag == "opt:build" and not row.tag.startswith("build")
    assert all(libraries.find(r.name) is r for r in libraries.ROWS)
    assert row.csrc.endswith("csrc_opt") and row.header.endswith("scsfm_opt.h") and row.lib.endswith("libscsfm_opt.so")
    assert row.prefix == "scsfm_opt_"
    assert "libscsfm_opt.so" in libraries.SUMMARY and "libscsfm_opt.so" in build.__doc__ and "libscsfm_opt.so" in _lib.__doc__
    assert build.OPT_LIB == row.lib and build.OPT_CSRC == row.csrc and _lib.OPT_HEADER == row.header
    assert _lib.OPT_LIB_PATH == row.lib and _lib.OPT_ABI_VERSION == 1 and callable(_lib.get_opt)
    assert [os.path.basename(p) for p in build.opt_sources()] == ["scsfm_adam.hip"]


def test_other_source_ids_do_not_see_csrc_opt():
    ids = []
    for row in libraries.TABLE + libraries.LATER:
        deps = build.lib_deps(row.name)
        assert deps and not any("csrc_opt" in p or "scsfm_opt" in p for p in deps), row.name
        ids.append(build.lib_source_id(row.name))
    assert all(os.sep + "csrc_opt" + os.sep in p or p.endswith("scsfm_opt.h") for p in build.opt_deps())
    assert len(set(ids)) == 17 and build.opt_source_id() not in ids


def test_header_declares_exactly_the_entry_points():
    assert set(_lib.parse_header(_lib.OPT_HEADER)) == ENTRY_POINTS
    text = open(_lib.OPT_HEADER).read()
    assert "#define SCSFM_OPT_CHUNK 2048" in text and "#define SCSFM_OPT_RECORD_BYTES 40" in text


def _lib_opt():
    return _lib.CLib(build.build_opt(verbose=False), _lib.OPT_HEADER, _lib.OPT_ABI_VERSION, "scsfm_opt_")


@needs_hipcc
def test_opt_library_builds_and_exports_its_header():
    path = build.build_opt(verbose=False)
    assert path.endswith("libscsfm_opt.so")
    assert build.binary_source_id(path) == build.opt_source_id() and not build.opt_is_stale()
    lib = _lib_opt()
    assert lib.source_id() == build.opt_source_id()
    assert lib._fn["scsfm_opt_abi_version"]() == 1
    assert set(lib.decls) == ENTRY_POINTS
    nm = shutil.which("nm") or "/opt/rocm/llvm/bin/llvm-nm"
    syms = subprocess.run([nm, "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in syms.splitlines() if " T " in line and "scsfm" in line}
    assert exported == ENTRY_POINTS
    assert _lib.get_opt().path == path


@needs_hipcc
def test_argument_errors_return_minus_one():
    lib = _lib_opt()
    p = ctypes.c_void_p(256)  # never dereferenced: every call below is rejected before anything is launched
    nan, inf = float("nan"), float("inf")
    fn = lib._fn["scsfm_opt_adam_step_f32"]
    #       table n_tensors map n_chunks exp_avg exp_avg_sq beta1 beta2 eps stream
    good = [p, 3, p, 5, p, p, 0.9, 0.999, 1e-8, None]
    odd8, odd16 = ctypes.c_void_p(260), ctypes.c_void_p(264)
    for k, bad in ((0, None), (2, None), (4, None), (5, None), (0, odd8), (2, odd8), (4, odd16), (5, odd16), (4, odd8),
                   (1, 0), (1, -1), (3, 0), (3, -1), (6, 1.0), (6, -0.1), (6, nan), (6, inf), (7, 1.0), (7, 1.5),
                   (7, -1e-9), (7, nan), (8, -1e-8), (8, nan), (8, inf), (8, -inf)):
        args = list(good)
        args[k] = bad
        assert fn(*args) == -1, (k, bad)
    assert lib._fn["scsfm_opt_source_id"](None, 64) == -1


def test_a_chunk_count_that_is_not_the_maps_length_is_refused(monkeypatch):
    """The library cannot see how long a map in device memory is (include/scsfm_opt.h): the optimiser, which writes the
    map, refuses to hand over a count that disagrees with it -- before the library is reached."""
    import torch

    from scsfm_hip import optim
    monkeypatch.setattr(optim, "_need_cuda", lambda *a: None)
    monkeypatch.setattr(_lib, "get_opt", lambda: pytest.fail("the library was reached"))
    params = [torch.nn.Parameter(torch.ones(5000)), torch.nn.Parameter(torch.ones(7))]
    opt = optim.Adam(params, lr=1e-3)
    assert len(opt._full_map) == 4
    for p in params:
        p.grad = torch.ones_like(p)
    opt._map = opt._map[:3]  # (a buffer laid out for fewer chunks than the tensors have)
    with pytest.raises(RuntimeError, match="chunk map"):
        opt.step()


@needs_hipcc
def test_no_kernel_spills_to_scratch(tmp_path):
    """The compiler's resource usage of the library's one kernel (read as tests/test_fbn_library.py reads it): no scratch,
    no LDS, and at most 64 vector registers so that eight waves per SIMD stay resident -- seven streams and no reuse: the
    kernel hides memory latency with occupancy.  Both access widths are in it."""
    out = tmp_path / "opt.s"
    flags = [f for f in build.FLAGS if f not in ("-shared", "-fPIC")]
    (src,) = build.opt_sources()
    subprocess.run([HIPCC, *flags, "-S", "--cuda-device-only", "-I", os.path.join(ROOT, "include"), "-o", str(out), src],
                   check=True, capture_output=True)
    text = open(out).read()
    kernels = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M)
    scratch = [int(x) for x in re.findall(r";\s*ScratchSize:\s*(\d+)", text)]
    vgprs = [int(x) for x in re.findall(r";\s*NumVgprs:\s*(\d+)", text)]
    lds = [int(x) for x in re.findall(r";\s*LDSByteSize:\s*(\d+)", text)]
    assert len(kernels) == 1 and len(scratch) == len(vgprs) == len(lds) == 1, (kernels, scratch)
    assert scratch == [0] and vgprs[0] <= 64 and lds == [0], (scratch, vgprs, lds)
    assert "global_load_dwordx4" in text and "global_store_dwordx4" in text and "global_load_dword " in text


@needs_hipcc
def test_build_reports_the_library_ahead_of_every_other_line(capsys):
    import sys
    sys.path.insert(0, ROOT)
    import __graft_entry__ as G
    G.build()
    out = capsys.readouterr().out.splitlines()
    mine = [i for i, line in enumerate(out) if line.startswith("[opt:build] ")]
    assert len(mine) == 1
    assert out[mine[0]] == f"[opt:build] {build.OPT_LIB}: {len(ENTRY_POINTS)} entry points resolved (ABI 1)"
    assert mine[0] == min(i for i, line in enumerate(out) if "entry points resolved" in line)
    reports = [i for i, line in enumerate(out) if line.endswith("entry points resolved")]
    assert len(reports) == 17 and out[reports[0]].startswith("[fbn:build] ")
    assert len([line for line in out if line.startswith("[build")]) == 10
    assert out[-2].startswith("[build:vis] ") and out[-1].startswith("[build:prep] ")
