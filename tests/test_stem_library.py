"""libscsfm_stem.so: builds with hipcc for gfx950 (no GPU needed), exports exactly the symbols include/scsfm_stem.h
declares, rejects bad arguments with -1 before touching any pointer, leaves the other five libraries' source ids alone,
and none of its kernels spills to scratch or needs more than 64 vector registers.  Also which inputs reach the fused
stem without a GPU: none."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest
import torch

from scsfm_hip import _lib, build

HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
needs_hipcc = pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc on this machine")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_other_source_ids_do_not_see_csrc_stem():
    others = build.deps() + build.nets_deps() + build.eval_deps() + build.odom_deps() + build.enc_deps()
    assert not any("csrc_stem" in p or "scsfm_stem" in p for p in others)
    assert build.stem_sources() and all(os.sep + "csrc_stem" + os.sep in p for p in build.stem_sources())
    assert all(os.sep + "csrc_stem" + os.sep in p or p.endswith("scsfm_stem.h") for p in build.stem_deps())
    ids = (build.source_id(), build.nets_source_id(), build.eval_source_id(), build.odom_source_id(),
           build.enc_source_id())
    assert build.stem_source_id() not in ids and len(set(ids)) == 5


def _lib_stem():
    return _lib.CLib(build.build_stem(verbose=False), _lib.STEM_HEADER, _lib.STEM_ABI_VERSION, "scsfm_stem_")


@needs_hipcc
def test_stem_library_builds_and_exports_its_header():
    path = build.build_stem(verbose=False)
    assert build.binary_source_id(path) == build.stem_source_id() and not build.stem_is_stale()
    lib = _lib_stem()
    assert lib.source_id() == build.stem_source_id()
    assert set(lib.decls) == {"scsfm_stem_abi_version", "scsfm_stem_source_id", "scsfm_stem_workspace_bytes",
                              "scsfm_stem_fwd_f32", "scsfm_stem_bwd_f32"}
    nm = shutil.which("nm") or "/opt/rocm/llvm/bin/llvm-nm"
    syms = subprocess.run([nm, "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in syms.splitlines() if " T " in line and "scsfm" in line}
    assert exported == set(lib.decls)
    assert _lib.get_stem().path == path


@needs_hipcc
def test_argument_errors_return_minus_one():
    lib = _lib_stem()
    p = ctypes.c_void_p(256)  # never dereferenced: every call below is rejected before anything is launched
    assert lib.size("scsfm_stem_workspace_bytes", 12, 64, 128, 416) >= 64 * 64 * 2 * 8
    assert lib.size("scsfm_stem_workspace_bytes", 1, 4, 1, 1) == 0  # one entry per channel: no variance
    assert lib.size("scsfm_stem_workspace_bytes", 0, 4, 2, 2) == 0
    assert lib.size("scsfm_stem_workspace_bytes", 64, 1024, 256, 256) == 0  # 2^32 elements
    n = lib.size("scsfm_stem_workspace_bytes", 2, 4, 3, 5)
    fn = lib._fn["scsfm_stem_fwd_f32"]
    good = [2, 4, 3, 5, 1e-5, 0.1, p, p, p, p, p, p, p, p, p, p, p, n, None]
    for k, bad in ((0, 0), (1, 0), (2, -1), (3, 0), (4, -1.0), (5, 1.5), (5, float("nan")), (6, None), (7, None),
                   (8, None), (9, None), (10, None), (11, None), (12, None), (13, None), (14, None), (15, None),
                   (16, None), (16, ctypes.c_void_p(260)), (17, n - 1)):
        args = list(good)
        args[k] = bad
        assert fn(*args) == -1, (k, bad)
    assert fn(1, 4, 1, 1, 1e-5, 0.1, p, p, p, p, p, p, p, p, p, p, p, 1 << 20, None) == -1
    fn = lib._fn["scsfm_stem_bwd_f32"]
    good = [2, 4, 3, 5, p, p, p, p, p, p, p, p, p, p, p, n, None]
    # (argument 5, g_f0, may be NULL: that is the variant without a gradient on f0)
    for k, bad in ((0, 0), (1, -3), (2, 0), (3, 0), (4, None), (6, None), (7, None), (8, None), (9, None), (10, None),
                   (11, None), (12, None), (13, None), (14, None), (14, ctypes.c_void_p(260)), (15, n - 1),
                   (0, 1 << 30)):
        args = list(good)
        args[k] = bad
        assert fn(*args) == -1, (k, bad)


@needs_hipcc
def test_no_kernel_spills_to_scratch(tmp_path):
    """The compiler's resource usage of every kernel of the library (read as tests/test_encoder_library.py reads it):
    no scratch, and at most 64 vector registers so that eight waves per SIMD stay resident."""
    out = tmp_path / "stem.s"
    flags = [f for f in build.FLAGS if f not in ("-shared", "-fPIC")]
    for src in build.stem_sources():
        subprocess.run([HIPCC, *flags, "-S", "--cuda-device-only", "-I", os.path.join(ROOT, "include"), "-o", str(out),
                        src], check=True, capture_output=True)
        text = open(out).read()
        kernels = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M)
        scratch = [int(x) for x in re.findall(r";\s*ScratchSize:\s*(\d+)", text)]
        vgprs = [int(x) for x in re.findall(r";\s*NumVgprs:\s*(\d+)", text)]
        # statistics x 2 widths, forward x 2 widths, the two backward launches x 2 widths x with / without g_f0
        assert len(kernels) == 12 and len(scratch) == len(kernels) == len(vgprs), (kernels, scratch)
        assert all(s == 0 for s in scratch), dict(zip(kernels, scratch))
        assert all(v <= 64 for v in vgprs), dict(zip(kernels, vgprs))


def _refuse(*a, **k):
    raise AssertionError("the fused stem was reached")


@pytest.mark.parametrize("variant", ["cpu_fp32_train", "cpu_fp32_eval", "cpu_fp64", "channels_last"])
def test_cpu_inputs_never_reach_the_fused_stem(variant, monkeypatch):
    from models.resnet_encoder import ResnetEncoder
    from scsfm_hip import encoder as E
    monkeypatch.setattr(E._BnReluPool, "apply", _refuse)
    monkeypatch.setattr(_lib, "get_stem", _refuse)
    dtype = torch.float64 if variant == "cpu_fp64" else torch.float32
    torch.manual_seed(0)
    enc = ResnetEncoder(18, False).to(dtype)
    enc.train(variant != "cpu_fp32_eval")
    x = torch.randn(2, 3, 32, 64, dtype=dtype)
    if variant == "channels_last":
        enc, x = enc.to(memory_format=torch.channels_last), x.contiguous(memory_format=torch.channels_last)
    state = {k: v.clone() for k, v in enc.state_dict().items()}
    got = enc(x)
    enc.load_state_dict(state)
    ref = enc.forward_reference(x)
    assert len(got) == len(ref) == 5 and all(torch.equal(a, b) for a, b in zip(got, ref))


def test_pool_needs_a_qualifying_call():
    import torch.nn as nn
    from scsfm_hip import encoder as E
    x = torch.randn(2, 4, 6, 6)
    with pytest.raises(ValueError):
        E.bn_act(x, nn.BatchNorm2d(4), pool=True)  # a CPU tensor
    with pytest.raises(ValueError):
        E.bn_act(x, nn.BatchNorm2d(4).eval(), pool=True)
