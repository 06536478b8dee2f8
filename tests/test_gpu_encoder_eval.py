"""The ResNet encoder's fused eval-mode glue (scsfm_hip.encoder_eval, csrc_enceval/scsfm_encoder_eval.hip) on the GPU
against the ATen chain it replaces: each op at the smallest shapes at which each path of the kernels can go wrong
(tests/_encoder_eval_ref.py), then whole encoders in eval mode under no_grad, which path the models take, graph capture,
and the way back to training mode.

The yardstick is the chain in fp64 with the fp32 chain measured beside it on the device:
max|fused32 - ref64| <= 2 max|aten32 - ref64| + 4 u max|ref64| per tensor.  The pooled map is exact: bit-identical to
F.max_pool2d of the kernel's own f0."""
import copy
import os
import subprocess
import sys
import textwrap

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import _encoder_eval_ref as R
from _util import report

pytestmark = pytest.mark.gpu

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "sc-sfmlearner-release_amd")
VECTORS = ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")


@pytest.fixture(autouse=True)
def _fused_eval_path(monkeypatch):
    monkeypatch.delenv("SCSFM_EVAL_TORCH", raising=False)


def _snapshot(bn):
    return [getattr(bn, k).detach().clone() for k in VECTORS]


def _unchanged(bn, before):
    return all(torch.equal(getattr(bn, k), b) for k, b in zip(VECTORS, before))


def _fused(case, pool=False):
    from scsfm_hip import encoder_eval as EE
    bn = R.eval_bn(case, torch.float32)
    before = _snapshot(bn)
    x = case["x"].float()
    identity = None if case["identity"] is None else case["identity"].float()
    with torch.no_grad():
        if pool:
            f0, pooled = EE.bn_act(x, bn, pool=True)
            out = dict(y=f0, pooled=pooled)
        else:
            out = dict(y=EE.bn_act(x, bn, identity, relu=case["mode"] != 0))
    assert _unchanged(bn, before), "a buffer or parameter of the module was written"
    assert all(not v.requires_grad and v.grad_fn is None for v in out.values())
    return out


@pytest.mark.parametrize("special", [False, True], ids=["finite", "nan_inf"])
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("shape", R.BN_SHAPES)
def test_bn_act_meets_the_contract(shape, mode, special):
    case = R.make_case(shape, mode, seed=sum(shape) + mode, device=DEV, special=special)
    fused = _fused(case)
    assert R.same_bits(fused["y"], _fused(case)["y"]), "two calls differ"
    if special:
        assert int(torch.isnan(fused["y"]).sum()) == 1 and bool(torch.isnan(fused["y"][0, 0, 0, 0]))
    R.check_eval_contract(f"gpu eval {R.MODES[mode]} {shape}", fused, R.aten_chain(case, torch.float32),
                          R.aten_chain(case, torch.float64))


@pytest.mark.parametrize("special", [False, True], ids=["finite", "nan_inf"])
@pytest.mark.parametrize("shape", R.POOL_SHAPES + [(1, 2, 5, 263), (1, 2, 9, 130)])
def test_stem_meets_the_contract_and_pools_its_own_f0(shape, special):
    from scsfm_hip import encoder_eval as EE
    case = R.make_case(shape, 1, seed=sum(shape), device=DEV, special=special)
    fused = _fused(case, pool=True)
    f0, pooled = fused["y"], fused["pooled"]
    assert R.same_bits(f0, _fused(case)["y"]), "f0 is not mode 1 of the plain kernel"
    assert R.same_bits(pooled, F.max_pool2d(f0, 3, 2, 1)), "pooled is not max_pool2d(f0)"
    with torch.no_grad():
        assert R.same_bits(pooled, EE.max_pool(f0)), "the plain pool differs from the fused one"
    R.check_eval_contract(f"gpu eval stem {shape}", fused, R.aten_chain(case, torch.float32, pool=True),
                          R.aten_chain(case, torch.float64, pool=True))


@pytest.mark.parametrize("shape", R.POOL_SHAPES + [(1, 1, 2, 3), (3, 2, 5, 263), (1, 4, 7, 131)])
def test_max_pool_is_bit_identical_to_aten(shape):
    from scsfm_hip import encoder_eval as EE
    gen = torch.Generator(device=DEV).manual_seed(sum(shape))
    x = torch.round(torch.randn(shape, device=DEV, generator=gen) * 2) / 2   # ties in most windows, negative entries
    x2 = x.clone()
    x2.view(-1)[::7] = float("nan")
    x2.view(-1)[3::11] = float("-inf")
    with torch.no_grad():
        for t in (x, x2):
            assert R.same_bits(EE.max_pool(t), F.max_pool2d(t, 3, 2, 1))


def _encoder(layers, images, seed):
    """an eval-mode encoder whose running statistics are not the initial 0 / 1, and its fp64 twin"""
    from models.resnet_encoder import ResnetEncoder
    torch.manual_seed(seed)
    enc = ResnetEncoder(layers, False, num_input_images=images).to(DEV)
    with torch.no_grad():
        for m in enc.modules():
            if isinstance(m, nn.BatchNorm2d):
                m.running_mean.normal_(0, 0.1)
                m.running_var.uniform_(0.5, 1.5)
                m.weight.uniform_(0.5, 1.5)
                m.bias.normal_(0, 0.1)
    enc.eval()
    return enc, copy.deepcopy(enc).double().eval()


def _count_calls(monkeypatch):
    from scsfm_hip import encoder as E, encoder_eval as EE
    calls = {"eval": 0, "train": 0}
    real_eval, real_train = EE.bn_act, E.bn_act

    def eval_bn_act(*a, **k):
        calls["eval"] += 1
        return real_eval(*a, **k)

    def train_bn_act(*a, **k):
        calls["train"] += 1
        return real_train(*a, **k)

    monkeypatch.setattr(EE, "bn_act", eval_bn_act)
    monkeypatch.setattr(E, "bn_act", train_bn_act)
    return calls


@pytest.fixture
def deterministic_miopen():
    old = torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = True, False
    yield
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = old


@pytest.mark.parametrize("layers,images,batch,n_calls", [(18, 1, 1, 20), (18, 1, 2, 20), (50, 1, 1, 53), (50, 1, 2, 53),
                                                         (18, 2, 1, 20)])
def test_whole_encoder_against_the_fp64_chain(layers, images, batch, n_calls, deterministic_miopen, monkeypatch):
    """Every feature map of the eval-mode encoder under no_grad: fused fp32 and forward_reference fp32, each against
    forward_reference in fp64, the same inequality per tensor; every BatchNorm went through encoder_eval.bn_act (20 of
    ResNet-18, 53 of ResNet-50), none through the training path; no buffer was written.  With SCSFM_EVAL_TORCH=1 no call
    arrives and the output is forward_reference's, bit for bit.  (images=2 is PoseResNet's encoder.)"""
    enc, enc64 = _encoder(layers, images, seed=layers + images)
    x = torch.randn(batch, 3 * images, 64, 96, device=DEV, generator=torch.Generator(device=DEV).manual_seed(batch))
    state = copy.deepcopy(enc.state_dict())
    calls = _count_calls(monkeypatch)
    with torch.no_grad():
        fused = enc(x)
        assert calls == {"eval": n_calls, "train": 0}, calls
        ref32 = enc.forward_reference(x)
        ref64 = enc64.forward_reference(x.double())
        assert calls == {"eval": n_calls, "train": 0}, calls
        monkeypatch.setenv("SCSFM_EVAL_TORCH", "1")
        plain = enc(x)
        assert calls == {"eval": n_calls, "train": 0}, calls
        assert all(R.same_bits(a, b) for a, b in zip(plain, ref32))
    assert all(torch.equal(state[k], v) for k, v in enc.state_dict().items()), "eval mode wrote a buffer"
    assert len(fused) == len(ref64) == 5
    R.check_contract(f"gpu eval ResnetEncoder({layers}) images={images} batch={batch}",
                     {f"f{i}": f for i, f in enumerate(fused)}, {f"f{i}": f for i, f in enumerate(ref32)},
                     {f"f{i}": f for i, f in enumerate(ref64)})


def test_pose_net_and_disp_net_take_the_eval_path(monkeypatch):
    import models
    calls = _count_calls(monkeypatch)
    torch.manual_seed(0)
    pose, disp = models.PoseResNet(18, False).to(DEV).eval(), models.DispResNet(18, False).to(DEV).eval()
    a, b = torch.randn(1, 3, 64, 96, device=DEV), torch.randn(1, 3, 64, 96, device=DEV)
    with torch.no_grad():
        p = pose(a, b)
        assert calls == {"eval": 20, "train": 0}, calls
        d = disp(a)
        assert calls == {"eval": 40, "train": 0}, calls
    assert p.shape == (1, 6) and bool(torch.isfinite(p).all())
    d = d[0] if isinstance(d, (list, tuple)) else d
    assert d.shape == (1, 1, 64, 96) and bool(torch.isfinite(d).all())


def test_eval_mode_with_grad_runs_the_aten_chain(deterministic_miopen, monkeypatch):
    enc, _ = _encoder(18, 1, seed=3)
    calls = _count_calls(monkeypatch)
    x = torch.randn(1, 3, 64, 96, device=DEV).requires_grad_()
    feats = enc(x)
    assert calls == {"eval": 0, "train": 0}, calls
    assert all(R.same_bits(a, b) for a, b in zip(feats, enc.forward_reference(x)))
    sum(f.sum() for f in feats).backward()
    grads = [p.grad for n, p in enc.named_parameters() if not n.startswith("encoder.fc.")]
    assert x.grad is not None and float(x.grad.abs().max()) > 0
    assert all(g is not None for g in grads) and float(enc.encoder.conv1.weight.grad.abs().max()) > 0


def test_training_mode_comes_back_after_an_eval_forward(deterministic_miopen, monkeypatch):
    """train -> eval forward -> train: the training-mode kernels are taken again and one forward + backward gives what it
    gave before, to 1e-5 of each tensor's scale (same state, same input and BatchNorm kernels with a fixed summation order:
    what is left is the convolutions' own reproducibility from run to run, a few fp32 roundings)."""
    enc, _ = _encoder(18, 1, seed=4)
    x = torch.randn(2, 3, 64, 96, device=DEV)
    state = copy.deepcopy(enc.state_dict())
    calls = _count_calls(monkeypatch)

    def train_step():
        enc.load_state_dict(state)
        enc.train()
        enc.zero_grad(set_to_none=True)
        feats = enc(x)
        sum((f * f).mean() for f in feats).backward()
        return ([f.detach().clone() for f in feats] + [enc.encoder.conv1.weight.grad.clone(),
                                                      enc.encoder.bn1.running_mean.clone()])

    first = train_step()
    assert calls == {"eval": 0, "train": 20}, calls
    enc.eval()
    with torch.no_grad():
        enc(x)
    assert calls == {"eval": 20, "train": 20}, calls
    second = train_step()
    assert calls == {"eval": 20, "train": 40}, calls
    for a, b in zip(first, second):
        err = float((a - b).abs().max())
        report(f"gpu train / eval / train: max |difference| {err:.3e} of {float(a.abs().max()):.3e}")
        assert err <= 1e-5 * float(a.abs().max())


CHILD = textwrap.dedent("""
    import sys, torch
    sys.path.insert(0, %r)
    from models.resnet_encoder import ResnetEncoder
    from scsfm_hip import encoder_eval as EE
    from scsfm_hip.graphs import GraphedStep
    torch.manual_seed(0)
    enc = ResnetEncoder(18, False).cuda().eval()
    x = torch.randn(1, 3, 64, 96, device="cuda")
    calls = []
    real = EE.bn_act
    EE.bn_act = lambda *a, **k: (calls.append(1), real(*a, **k))[1]

    def step():
        with torch.no_grad():
            return enc(x)

    eager = [f.clone() for f in step()]
    assert len(calls) == 20, len(calls)
    g = GraphedStep(step)
    got = g.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(got, eager)), "replay vs eager"
    x.mul_(1.5)                               # new data in the same tensor
    got = [f.clone() for f in g.replay()]
    want = step()
    torch.cuda.synchronize()
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(got, want)), "replay after update"
    assert not torch.equal(got[4], eager[4])
    print("GRAPH-OK")
""") % PKG


def test_eval_forward_captured_in_a_graph_gives_the_eager_bits():
    """(in a child process, as tests/test_gpu_graph.py: a failure inside graph capture can take the interpreter down)"""
    env = dict(os.environ, PYTHONPATH=PKG)
    env.pop("SCSFM_EVAL_TORCH", None)
    out = subprocess.run([sys.executable, "-c", CHILD], capture_output=True, text=True, timeout=600, env=env)
    assert out.returncode == 0 and "GRAPH-OK" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
