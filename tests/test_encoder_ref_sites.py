"""The yardstick's own helpers (tests/_encoder_ref.py) on the CPU: the functional walk over the ReLU sites is the chain
that ResnetEncoder.forward_reference runs, for BasicBlock and Bottleneck; conditioning the ResNet-18 encoder gives what
it gave before the walk learnt about Bottlenecks; a single Bottleneck can be conditioned, and the fp32 error of its
pre-activations leaves KINK_MARGIN the room the GPU test asks for."""
import copy

import pytest
import torch
import torch.nn.functional as F

import _encoder_ref as R


def _encoder(layers, seed):
    from models.resnet_encoder import ResnetEncoder
    torch.manual_seed(seed)
    return ResnetEncoder(layers, False).train()


@pytest.mark.parametrize("layers,n_sites,per_block", [(18, 17, 2), (50, 49, 3)])
def test_the_site_walk_is_the_reference_chain(layers, n_sites, per_block):
    enc64 = _encoder(layers, 0).double()
    x = torch.randn(2, 3, 32, 64, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    with torch.no_grad():
        sites = list(R._relu_sites(enc64, x))
        feats = enc64.forward_reference(x)
    assert len(sites) == n_sites
    e = enc64.encoder
    convs = [e.conv1] + [getattr(b, f"conv{k + 1}") for layer in (e.layer1, e.layer2, e.layer3, e.layer4) for b in layer
                         for k in range(per_block)]
    assert all(a is b for a, (b, _, _) in zip(convs, sites))
    assert sites[0][2] is not None and all(s[2] is None for s in sites[1:])
    ends, k = [0], 0
    for layer in (e.layer1, e.layer2, e.layer3, e.layer4):
        k += per_block * len(layer)
        ends.append(k)
    for f, k in zip(feats, ends):  # the ReLU of the site that ends a stage is the stage's feature map
        assert float((F.relu(sites[k][1]) - f).abs().max()) <= 1e-12 * float(f.abs().max())


def test_resnet18_conditioning_is_what_it_was():
    """seeds and inputs of test_gpu_encoder_fused.test_whole_encoder_against_the_fp64_chain[1-1] with torch-CPU's
    generator; 45 re-draws and these margins are what the walk over BasicBlocks alone gave"""
    enc64 = _encoder(18, 1).double()
    gen = torch.Generator().manual_seed(3)
    xs = [torch.randn(2, 3, 64, 128, generator=gen).double()]
    rounds, lo_v, lo_gap = R.condition_encoder(enc64, xs, seed=6)
    assert rounds == 45
    assert lo_v == pytest.approx(0.0003007458133635064, rel=1e-9)
    assert lo_gap == pytest.approx(0.00030785808796851555, rel=1e-9)


@pytest.mark.parametrize("layer,index,shape", [(1, 0, (2, 64, 16, 32)), (4, 1, (2, 2048, 2, 4))])
def test_a_bottleneck_can_be_conditioned_alone(layer, index, shape):
    block = copy.deepcopy(getattr(_encoder(50, 50).encoder, f"layer{layer}")[index])
    gen = torch.Generator().manual_seed(layer)
    xs = [torch.relu(torch.randn(shape, generator=gen)) for _ in range(3)]
    block64 = copy.deepcopy(block).double()
    before = copy.deepcopy(block64.state_dict())
    rounds, lo_v, lo_gap = R.condition_encoder(block64, [x.double() for x in xs], seed=2, sites=R.block_sites)
    assert rounds < 100 and lo_v >= R.KINK_MARGIN and lo_gap == float("inf")
    changed = [n for n, t in block64.state_dict().items() if not torch.equal(t, before[n])]
    assert all(n in ("conv1.weight", "conv2.weight", "conv3.weight") for n in changed)  # (never the down-sample branch)
    block.load_state_dict(block64.state_dict())
    assert all(torch.equal(a.double(), b) for a, b in zip(block.state_dict().values(), block64.state_dict().values()))
    errs = R.preactivation_errors(block, block64, xs, R.block_sites)
    assert len(errs) == 3 and 0 < max(errs) == R.preactivation_error(block, block64, xs, R.block_sites)
    assert R.KINK_MARGIN >= 10 * max(errs)
