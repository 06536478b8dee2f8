"""Which path DepthDecoder.forward takes now that the biases can be folded into the glue (forward_fused_bias), without a
GPU: CPU, fp64 and channels_last inputs keep the reference chain, SCSFM_DECODER_BIAS=0 selects forward_fused, the module
tree and the state dict are the reference's, and a frozen bias gets no gradient and costs no reduction."""
import pytest
import torch

import _hostsim_decb as HB
import _hostsim_nets as HS


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

    def refuse(self, feats):
        raise AssertionError("a fused path was taken")
    monkeypatch.setattr(DepthDecoder, "forward_fused", refuse)
    monkeypatch.setattr(DepthDecoder, "forward_fused_bias", refuse)
    with torch.no_grad():
        out = net(x)
        ref = net.decoder.forward_reference(net.encoder(x))[0]
    assert torch.equal(out, ref)


def _dispatch(monkeypatch, env, biases_ok=True):
    """the path forward() takes when the fused path applies"""
    from models.DispResNet import DepthDecoder
    from scsfm_hip import config
    if env is None:
        monkeypatch.delenv("SCSFM_DECODER_BIAS", raising=False)
    else:
        monkeypatch.setenv("SCSFM_DECODER_BIAS", env)
    monkeypatch.setattr(config, "_decoder_bias", None)  # (read once: read again)
    dec = DepthDecoder([4, 4, 8, 8, 16])
    monkeypatch.setattr(DepthDecoder, "fused_path_applies", lambda self, feats: True)
    if biases_ok:  # (the biases of this CPU module stand in for CUDA ones)
        monkeypatch.setattr(DepthDecoder, "bias_path_applies", lambda self: config.decoder_bias_folded())
    monkeypatch.setattr(DepthDecoder, "forward_fused", lambda self, feats: "fused")
    monkeypatch.setattr(DepthDecoder, "forward_fused_bias", lambda self, feats: "fused_bias")
    monkeypatch.setattr(DepthDecoder, "forward_reference", lambda self, feats: "reference")
    return dec.forward([])


def test_the_environment_switch_selects_forward_fused(monkeypatch):
    assert _dispatch(monkeypatch, None) == "fused_bias"
    assert _dispatch(monkeypatch, "1") == "fused_bias"
    assert _dispatch(monkeypatch, "0") == "fused"


def test_biases_that_are_not_cuda_fp32_take_forward_fused(monkeypatch):
    """bias_path_applies itself: CPU biases (and a convolution without one) do not qualify, whatever the switch says"""
    from models.DispResNet import DepthDecoder
    assert _dispatch(monkeypatch, "1", biases_ok=False) == "fused"
    dec = DepthDecoder([4, 4, 8, 8, 16])
    assert not dec.bias_path_applies()
    dec._conv(3).bias = None
    assert not dec.bias_path_applies()


def test_config_switch_is_read_once_and_can_be_set(monkeypatch):
    from scsfm_hip import config
    monkeypatch.setattr(config, "_decoder_bias", None)
    monkeypatch.setenv("SCSFM_DECODER_BIAS", "0")
    assert config.decoder_bias_folded() is False
    monkeypatch.setenv("SCSFM_DECODER_BIAS", "1")
    assert config.decoder_bias_folded() is False
    config.set_decoder_bias_folded(True)
    assert config.decoder_bias_folded() is True


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
    assert [n for n, _ in dec.named_children()] == ["decoder", "sigmoid"] and len(dec.decoder) == 14


def test_a_frozen_bias_gets_no_gradient_and_no_reduction(monkeypatch):
    """forward_fused_bias on the simulator with the biases of conv (2, 1) and of head 0 frozen: both stay without a
    gradient, every other bias on the path of scale 0 gets one, and the number of bias sums that ran is the number of
    biases that wanted a gradient (ctx.needs_input_grad decides)."""
    from models.DispResNet import DepthDecoder
    from scsfm_hip import decoder as D, decoder_bias as DB
    monkeypatch.setattr(D, "pad", HS.pad)
    for name in ("elu_pad", "up_cat_pad", "disp_head"):
        monkeypatch.setattr(DB, name, getattr(HB, name))
    torch.manual_seed(3)
    dec = DepthDecoder([4, 4, 8, 8, 16])
    frozen = [dec._conv(dec._up[(2, 1)]).bias, dec._conv(dec._head[0]).bias]
    for b in frozen:
        b.requires_grad_(False)
    feats = [torch.randn(1, c, 2 << (4 - k), 3 << (4 - k)) for k, c in enumerate([4, 4, 8, 8, 16])]
    monkeypatch.setattr(HB, "REDUCTIONS", [0])
    outs = dec.forward_fused_bias(feats)
    outs[0].sum().backward()
    assert all(b.grad is None for b in frozen)
    live = [dec._conv(k).bias for k in range(10) if dec._conv(k).bias is not frozen[0]]
    assert len(live) == 9 and all(b.grad is not None and b.grad.shape == b.shape for b in live)
    assert all(dec._conv(dec._head[s]).bias.grad is None for s in (1, 2, 3))  # (their outputs are not in the loss)
    assert HB.REDUCTIONS[0] == 9
    # nothing requires a gradient: no reduction at all
    for p in dec.parameters():
        p.requires_grad_(False)
    monkeypatch.setattr(HB, "REDUCTIONS", [0])
    feats = [f.requires_grad_() for f in feats]
    dec.forward_fused_bias(feats)[0].sum().backward()
    assert HB.REDUCTIONS[0] == 0 and all(f.grad is not None for f in feats)
