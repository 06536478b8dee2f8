"""libscsfm_vlog.so: the header parses to exactly its entry points, the library builds with hipcc for gfx950 (no GPU
needed), exports those symbols and nothing else, carries the ABI version and the tree's source id, leaves the other
libraries' source ids alone, rejects bad arguments with -1 before anything is launched, and none of its kernels spills
to scratch or contracts the input picture's multiply and add; build() reports it under its own tag ahead of the
"[build" lines."""
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
ENTRY_POINTS = {"scsfm_vlog_abi_version", "scsfm_vlog_source_id", "scsfm_vlog_input_picture",
                "scsfm_vlog_target_disparity", "scsfm_vlog_image_max", "scsfm_vlog_map_picture"}
OTHERS = ("", "nets_", "eval_", "odom_", "enc_", "stem_", "snip_", "prep_", "vis_", "dvis_", "val_", "enceval_",
          "decb_", "wrw_")


def test_other_source_ids_do_not_see_csrc_vlog():
    for prefix in OTHERS:
        deps = getattr(build, prefix + "deps")()
        assert deps and not any("csrc_vlog" in p or "scsfm_vlog" in p for p in deps), prefix
    assert build.vlog_sources() and all(os.sep + "csrc_vlog" + os.sep in p for p in build.vlog_sources())
    assert all(os.sep + "csrc_vlog" + os.sep in p or p.endswith("scsfm_vlog.h") for p in build.vlog_deps())
    ids = [getattr(build, prefix + "source_id")() for prefix in OTHERS]
    assert len(set(ids)) == len(OTHERS) and build.vlog_source_id() not in ids


def test_header_declares_exactly_the_entry_points():
    decls = _lib.parse_header(_lib.VLOG_HEADER)
    assert set(decls) == ENTRY_POINTS
    i, p, d = ctypes.c_int, ctypes.c_void_p, ctypes.c_double
    assert decls["scsfm_vlog_input_picture"] == (i, [i, i, i, p, p, p, p])
    assert decls["scsfm_vlog_target_disparity"] == decls["scsfm_vlog_image_max"] == (i, [i, i, p, p, p])
    assert decls["scsfm_vlog_map_picture"] == (i, [i, i, i, p, p, i, p, d, p, p, p])
    assert _lib.VLOG_ABI_VERSION == 1


def test_gitignore_names_the_library_temporaries():
    lines = open(os.path.join(ROOT, ".gitignore")).read().split()
    assert "libscsfm_vlog.*.tmp" in lines and "*.so" in lines


def _lib_vlog():
    return _lib.CLib(build.build_vlog(verbose=False), _lib.VLOG_HEADER, _lib.VLOG_ABI_VERSION, "scsfm_vlog_")


@needs_hipcc
def test_vlog_library_builds_and_exports_its_header():
    path = build.build_vlog(verbose=False)
    assert path.endswith("libscsfm_vlog.so")
    assert build.binary_source_id(path) == build.vlog_source_id() and not build.vlog_is_stale()
    lib = _lib_vlog()
    assert lib.source_id() == build.vlog_source_id()
    assert lib._fn["scsfm_vlog_abi_version"]() == _lib.VLOG_ABI_VERSION == 1
    assert set(lib.decls) == ENTRY_POINTS
    nm = shutil.which("nm") or "/opt/rocm/llvm/bin/llvm-nm"
    syms = subprocess.run([nm, "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in syms.splitlines() if " T " in line and "scsfm" in line}
    assert exported == ENTRY_POINTS
    assert _lib.get_vlog().path == path


@needs_hipcc
def test_argument_errors_return_minus_one():
    lib = _lib_vlog()
    p = ctypes.c_void_p(256)  # never dereferenced: every call below is rejected before anything is launched
    odd = ctypes.c_void_p(258)
    off16 = ctypes.c_void_p(260)
    fn = lib._fn["scsfm_vlog_input_picture"]
    #       N  H  W  in out_f out_u8 stream
    good = [2, 5, 7, p, p, p, None]
    for k, bad in ((0, 0), (0, -1), (1, 0), (2, 0), (3, None), (3, odd), (4, odd), (0, 1 << 29)):
        args = list(good)
        args[k] = bad
        assert fn(*args) == -1, (k, bad)
    assert fn(2, 5, 7, p, None, None, None) == -1  # no output at all

    for name in ("scsfm_vlog_target_disparity", "scsfm_vlog_image_max"):
        fn = lib._fn[name]
        #       N  HW  in out stream
        good = [3, 35, p, p, None]
        for k, bad in ((0, 0), (1, 0), (1, -3), (2, None), (2, odd), (3, None), (3, odd), (1, 1 << 28)):
            args = list(good)
            args[k] = bad
            assert fn(*args) == -1, (name, k, bad)

    fn = lib._fn["scsfm_vlog_map_picture"]
    #       N  H  W  in table n     divisors max out_f out_u8 stream
    good = [3, 5, 7, p, p, 1000, p, 0.0, p, p, None]
    for k, bad in ((0, 0), (1, 0), (2, -1), (3, None), (3, odd), (4, None), (4, odd), (4, off16), (5, 0), (5, -1),
                   (5, (1 << 24) + 1), (6, odd), (8, odd), (9, odd), (0, 1 << 25)):
        args = list(good)
        args[k] = bad
        assert fn(*args) == -1, (k, bad)
    assert fn(3, 5, 7, p, p, 1000, p, 0.0, None, None, None) == -1  # no output at all
    assert lib._fn["scsfm_vlog_source_id"](None, 64) == -1


@needs_hipcc
def test_no_kernel_spills_and_the_input_picture_is_not_contracted(tmp_path):
    """The compiler's resource usage of every kernel (read as tests/test_vis_library.py reads it), and the body of the
    input picture's kernel, whose only float arithmetic is x * 0.225f, 0.45f + . and 255.0f * .: no fused multiply-add."""
    out = tmp_path / "vlog.s"
    flags = [f for f in build.FLAGS if f not in ("-shared", "-fPIC")]
    n = 0
    for src in build.vlog_sources():
        subprocess.run([HIPCC, *flags, "-S", "--cuda-device-only", "-I", os.path.join(ROOT, "include"), "-o", str(out),
                        src], check=True, capture_output=True)
        text = open(out).read()
        kernels = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M)
        scratch = [int(x) for x in re.findall(r";\s*ScratchSize:\s*(\d+)", text)]
        assert len(scratch) == len(kernels), (kernels, scratch)
        assert all(s == 0 for s in scratch), dict(zip(kernels, scratch))
        (name,) = [k for k in kernels if "input_kernel" in k]
        body = text.split(name + ":", 1)[1].split("s_endpgm", 1)[0]
        assert "v_mul_f32" in body and "v_add_f32" in body
        assert not re.search(r"\bv_(pk_)?(fma|fmac|mad|mac)_(f32|legacy_f32)\b", body)
        n += len(kernels)
    # input; target; maximum, decode; map
    assert n == 5


@needs_hipcc
def test_build_reports_the_library_ahead_of_the_build_lines(capsys):
    import sys
    sys.path.insert(0, ROOT)
    import __graft_entry__ as G
    G.build()
    out = capsys.readouterr().out.splitlines()
    mine = [i for i, line in enumerate(out) if line.startswith("[vlog:build] ")]
    assert len(mine) == 1
    assert out[mine[0]] == f"[vlog:build] {build.VLOG_LIB}: {len(ENTRY_POINTS)} entry points resolved"
    first = min(i for i, line in enumerate(out) if line.startswith("[build"))
    assert mine[0] < first and len([line for line in out if line.startswith("[build")]) == 10


def test_wrappers_refuse_host_tensors_and_unknown_maps():
    import torch
    from scsfm_hip import validation_log as VL
    with pytest.raises(RuntimeError):
        VL.map_pictures(torch.ones(1, 4, 4))
    with pytest.raises(RuntimeError):
        VL.image_max(torch.ones(1, 4, 4))
    with pytest.raises(RuntimeError):
        VL.target_disparity(torch.ones(1, 4, 4))
    with pytest.raises(RuntimeError):
        VL.input_pictures(torch.zeros(1, 3, 4, 4))
    with pytest.raises(RuntimeError):
        VL.tensor2array(torch.ones(4, 4))
    for name in ("viridis", ""):
        with pytest.raises(ValueError):
            VL.colour_table_f32(name)
        with pytest.raises(ValueError):
            VL.map_pictures(torch.ones(1, 4, 4), colormap=name)
