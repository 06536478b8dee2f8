"""The depth decoder's fused glue without a GPU: which path DepthDecoder.forward takes, that the module tree and state
dict are those of the reference, and that libscsfm_nets.so builds with hipcc, exports every symbol its header declares
and compiles to kernels that spill nothing."""
import os
import re
import shutil
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def _net(dtype=torch.float32):
    import models
    torch.manual_seed(0)
    return models.DispResNet(18, False).to(dtype)


@pytest.mark.parametrize("variant", ["cpu_fp32", "cpu_fp64", "channels_last"])
def test_cpu_fp64_and_channels_last_take_the_reference_chain(variant, monkeypatch):
    from models.DispResNet import DepthDecoder
    dtype = torch.float64 if variant == "cpu_fp64" else torch.float32
    net = _net(dtype).eval()
    x = torch.randn(1, 3, 64, 96, dtype=dtype)
    if variant == "channels_last":
        net, x = net.to(memory_format=torch.channels_last), x.contiguous(memory_format=torch.channels_last)
    feats = net.encoder(x)
    assert not net.decoder.fused_path_applies(feats)

    def refuse(self, feats):
        raise AssertionError("the fused path was taken")
    monkeypatch.setattr(DepthDecoder, "forward_fused", refuse)
    with torch.no_grad():
        out = net(x)
        ref = net.decoder.forward_reference(net.encoder(x))[0]
    assert torch.equal(out, ref)


def test_state_dict_and_module_tree_unchanged():
    net = _net()
    keys = [k for k in net.state_dict() if k.startswith("decoder.")]
    want = []
    for k in range(14):
        p = f"decoder.decoder.{k}.conv.conv" if k < 10 else f"decoder.decoder.{k}.conv"
        want += [p + ".weight", p + ".bias"]
    assert keys == want
    dec = net.decoder
    assert dec._up == {(i, j): 2 * (4 - i) + j for i in range(5) for j in range(2)}
    assert dec._head == {s: 10 + s for s in range(4)}


def test_nets_library_builds_and_exports_its_header():
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc on this machine")
    from scsfm_hip import _lib, build
    path = build.build_nets(verbose=False)
    assert build.binary_source_id(path) == build.nets_source_id()
    lib = _lib.CLib(path, _lib.NETS_HEADER, _lib.NETS_ABI_VERSION, "scsfm_nets_")
    assert set(lib.decls) == {"scsfm_nets_abi_version", "scsfm_nets_source_id", "scsfm_nets_pad_fwd_f32",
                              "scsfm_nets_pad_bwd_f32", "scsfm_nets_up_cat_pad_fwd_f32", "scsfm_nets_up_cat_pad_bwd_f32"}
    assert lib.source_id() == build.nets_source_id()
    # the loss library's id does not cover the nets' sources
    assert not any("csrc_nets" in p or "scsfm_nets" in p for p in build.deps())
    # rejected arguments come back as -1 before anything is launched
    assert lib._fn["scsfm_nets_pad_fwd_f32"](1, 1, 1, 4, 0, None, None, None) == -1
    assert lib._fn["scsfm_nets_up_cat_pad_bwd_f32"](1, 2, 3, 4, 4, None, None, None, None, None) == -1


def test_nets_kernels_spill_nothing(tmp_path):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc on this machine")
    from scsfm_hip import build
    flags = [f for f in build.FLAGS if f not in ("-shared", "-fPIC")]
    r = subprocess.run([HIPCC, *flags, "-c", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-I",
                        build.INCLUDE, "-o", str(tmp_path / "dec.o"), *build.nets_sources()],
                       check=True, capture_output=True, text=True)
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    vgprs = [int(v) for v in re.findall(r"\bVGPRs: (\d+)", r.stderr)]
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    occupancy = [int(v) for v in re.findall(r"Occupancy \[waves/SIMD\]: (\d+)", r.stderr)]
    assert len(names) == 6 and len(vgprs) == len(scratch) == len(occupancy) == 6, r.stderr[-2000:]
    assert all(s == 0 for s in scratch) and max(vgprs) <= 64 and min(occupancy) == 8, (names, vgprs, occupancy)
