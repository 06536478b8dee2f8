"""libscsfm_vis.so: builds with hipcc for gfx950 (no GPU needed), exports exactly the symbols include/scsfm_vis.h
declares, rejects bad arguments with -1 before touching any pointer, leaves the other eight libraries' source ids alone,
and none of its kernels spills to scratch."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import pytest

from scsfm_hip import _lib, build, visualise

HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
needs_hipcc = pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc on this machine")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_other_source_ids_do_not_see_csrc_vis():
    others = build.deps() + build.nets_deps() + build.eval_deps() + build.odom_deps() + build.enc_deps() + \
        build.stem_deps() + build.snip_deps() + build.prep_deps()
    assert not any("csrc_vis" in p or "scsfm_vis" in p for p in others)
    assert build.vis_sources() and all(os.sep + "csrc_vis" + os.sep in p for p in build.vis_sources())
    assert all(os.sep + "csrc_vis" + os.sep in p or p.endswith("scsfm_vis.h") for p in build.vis_deps())
    ids = (build.source_id(), build.nets_source_id(), build.eval_source_id(), build.odom_source_id(),
           build.enc_source_id(), build.stem_source_id(), build.snip_source_id(), build.prep_source_id())
    assert build.vis_source_id() not in ids and len(set(ids)) == 8


def _lib_vis():
    return _lib.CLib(build.build_vis(verbose=False), _lib.VIS_HEADER, _lib.VIS_ABI_VERSION, "scsfm_vis_")


@needs_hipcc
def test_vis_library_builds_and_exports_its_header():
    path = build.build_vis(verbose=False)
    assert build.binary_source_id(path) == build.vis_source_id() and not build.vis_is_stale()
    lib = _lib_vis()
    assert lib.source_id() == build.vis_source_id()
    assert lib._fn["scsfm_vis_abi_version"]() == _lib.VIS_ABI_VERSION == 1
    assert set(lib.decls) == {"scsfm_vis_abi_version", "scsfm_vis_source_id", "scsfm_vis_normalise_u8",
                              "scsfm_vis_image_max", "scsfm_vis_colourise"}
    nm = shutil.which("nm") or "/opt/rocm/llvm/bin/llvm-nm"
    syms = subprocess.run([nm, "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in syms.splitlines() if " T " in line and "scsfm" in line}
    assert exported == set(lib.decls)
    assert _lib.get_vis().path == path


@needs_hipcc
def test_build_resolves_the_ninth_library_before_the_last_line(capsys):
    """build() reports libscsfm_vis.so under its own tag, once, after the seven "[build] " lines and before the
    "[build:prep] " line, which stays last."""
    sys.path.insert(0, ROOT)
    import __graft_entry__ as G
    G.build()
    out = capsys.readouterr().out.splitlines()
    assert [line.split("/")[-1].split(":")[0] for line in out if line.startswith("[build] ")] == [
        "libscsfm_hip.so", "libscsfm_nets.so", "libscsfm_eval.so", "libscsfm_odom.so", "libscsfm_enc.so",
        "libscsfm_stem.so", "libscsfm_snip.so"]
    mine = [i for i, line in enumerate(out) if line.startswith("[build:vis] ")]
    assert len(mine) == 1
    assert out[mine[0]] == f"[build:vis] {build.VIS_LIB}: {len(_lib.parse_header(_lib.VIS_HEADER))} entry points resolved"
    assert out[mine[0]].endswith(": 5 entry points resolved")
    assert out[mine[0] - 1].startswith("[build] ") and "libscsfm_snip.so" in out[mine[0] - 1]
    assert mine[0] == len(out) - 2 and out[-1].startswith("[build:prep] ")


@needs_hipcc
def test_argument_errors_return_minus_one():
    lib = _lib_vis()
    p = ctypes.c_void_p(256)  # never dereferenced: every call below is rejected before anything is launched
    odd = ctypes.c_void_p(258)
    fn = lib._fn["scsfm_vis_normalise_u8"]
    #       N  H  W  in out stream
    good = [2, 5, 7, p, p, None]
    for k, bad in ((0, 0), (0, -1), (1, 0), (2, 0), (3, None), (4, None), (4, odd), (0, 1 << 29)):
        args = list(good)
        args[k] = bad
        assert fn(*args) == -1, (k, bad)

    fn = lib._fn["scsfm_vis_image_max"]
    #       N  HW  in out stream
    good = [3, 35, p, p, None]
    for k, bad in ((0, 0), (1, 0), (1, -3), (2, None), (2, odd), (3, None), (3, odd), (1, 1 << 28)):
        args = list(good)
        args[k] = bad
        assert fn(*args) == -1, (k, bad)

    fn = lib._fn["scsfm_vis_colourise"]
    #       N  H  W  in table n     divisors max  rec out stream
    good = [3, 5, 7, p, p, 1000, p, 0.0, 0, p, None]
    for k, bad in ((0, 0), (1, 0), (2, -1), (3, None), (3, odd), (4, None), (4, odd), (5, 0), (5, -1), (5, (1 << 24) + 1),
                   (6, odd), (9, None), (9, odd), (0, 1 << 25)):
        args = list(good)
        args[k] = bad
        assert fn(*args) == -1, (k, bad)
    assert lib._fn["scsfm_vis_source_id"](None, 64) == -1


@needs_hipcc
def test_no_kernel_spills_to_scratch(tmp_path):
    """The compiler's resource usage of every kernel of the library (read as tests/test_prep_library.py reads it)."""
    out = tmp_path / "vis.s"
    flags = [f for f in build.FLAGS if f not in ("-shared", "-fPIC")]
    n = 0
    for src in build.vis_sources():
        subprocess.run([HIPCC, *flags, "-S", "--cuda-device-only", "-I", os.path.join(ROOT, "include"), "-o", str(out),
                        src], check=True, capture_output=True)
        text = open(out).read()
        kernels = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M)
        scratch = [int(x) for x in re.findall(r";\s*ScratchSize:\s*(\d+)", text)]
        vgprs = [int(x) for x in re.findall(r";\s*NumVgprs:\s*(\d+)", text)]
        assert len(scratch) == len(kernels) == len(vgprs), (kernels, scratch)
        assert all(s == 0 for s in scratch), dict(zip(kernels, scratch))
        assert all(v <= 128 for v in vgprs), dict(zip(kernels, vgprs))
        # the pictures go through 16-byte accesses, and every division is the full one (no bare reciprocal multiply)
        assert "global_load_dwordx4" in text and "global_store_dwordx4" in text
        assert len(re.findall(r"v_div_fixup_f32", text)) >= 9
        n += len(kernels)
    # normalise; maximum, decode; colourise
    assert n == 4


def test_colour_table_names():
    assert visualise.colour_table("bone").shape == (10000, 4) and visualise.colour_table("rainbow").shape == (1000, 4)
    assert visualise.colour_table("bone") is visualise.colour_table("bone")  # cached
    assert not visualise.colour_table("bone").flags.writeable
    for name in ("magma", "viridis", ""):
        with pytest.raises(ValueError):
            visualise.colour_table(name)


def test_wrappers_refuse_host_tensors():
    import torch
    with pytest.raises(RuntimeError):
        visualise.colourise(torch.ones(1, 4, 4))
    with pytest.raises(RuntimeError):
        visualise.image_max(torch.ones(1, 4, 4))
    with pytest.raises(RuntimeError):
        visualise.normalise_u8(torch.zeros(1, 4, 4, 3, dtype=torch.uint8))
    with pytest.raises(ValueError):
        visualise.colourise(torch.ones(1, 4, 4), colormap="magma")
