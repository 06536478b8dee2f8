"""libscsfm_opt.so and scsfm_hip.optim.Adam on the device: the host simulator's case list bit for bit against the same
numpy restatement of include/scsfm_opt.h; smoke()'s shapes; a run split through state_dict() and a file; and agreement with
torch.optim.Adam on the parameter lists of both nets, each measured against an fp64 Adam on the host."""
import numpy as np
import pytest
import torch

import _adam_cases as C

pytestmark = pytest.mark.gpu
# ulp of the parameter allowed on top of twice torch's own error: five final subtractions of half an ulp each, rounded up
# (test_agreement_with_torch_on_both_nets; measured on the MI355X: none needed, worst ratio to torch's error 1.69)
ULPS = 3


class DeviceBackend:
    """arenas on the device (torch's allocations start on 512-byte boundaries)"""

    def __init__(self):
        self.dev = torch.device("cuda:0")
        self.stream = None  # the null stream: torch's current stream unless a test changes it

    def upload(self, a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)

    def write(self, h, a):
        h.copy_(torch.from_numpy(a))

    def ptr(self, h):
        return h.data_ptr()

    def download(self, h):
        torch.cuda.synchronize()
        return h.cpu().numpy()


def _lib_opt():
    from scsfm_hip import _lib
    return _lib.get_opt()


@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_five_steps_equal_the_numpy_restatement_bit_for_bit(wd):
    tensors = C.default_tensors()
    steps = C.run_case(_lib_opt(), DeviceBackend(), tensors, wd)
    assert sorted(set(steps)) == [C.STEPS - len(C.ABSENT_IN), C.STEPS]


def test_the_smoke_shapes():
    import sys
    import os
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import __graft_entry__ as G
    C.run_case(_lib_opt(), DeviceBackend(), C.smoke_tensors(), 0.0, steps=3, absent_in=())
    G._smoke_opt(torch.device("cuda:0"))


def _recorded(shapes, steps, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(s, generator=g) for s in shapes], [[torch.randn(s, generator=g) for s in shapes] for _ in range(steps)]


def _make(init, dev):
    from scsfm_hip import optim
    params = [torch.nn.Parameter(t.to(dev)) for t in init]
    half = len(params) // 2
    return params, optim.Adam([{"params": params[:half], "lr": 1e-3}, {"params": params[half:], "lr": 1e-2}],
                              betas=(0.9, 0.999), weight_decay=0.01)


def _steps(params, opt, grads, skip=None):
    for gs in grads:
        for k, (p, g) in enumerate(zip(params, gs)):
            p.grad = None if k == skip else g.to(p.device)
        opt.step()


def test_a_run_split_through_a_state_file_equals_the_straight_run(tmp_path):
    dev = torch.device("cuda:0")
    shapes = [(5, 3), (C.CHUNK + 1,), (7,), (2, 3, 3, 3), (4,)]
    init, grads = _recorded(shapes, 4, 21)
    pa, oa = _make(init, dev)
    _steps(pa, oa, grads, skip=4)  # (the last tensor never has a gradient)
    pb, ob = _make(init, dev)
    _steps(pb, ob, grads[:2], skip=4)
    torch.save(ob.state_dict(), tmp_path / "opt.pth")
    pc, oc = _make([p.detach().cpu() for p in pb], dev)
    oc.load_state_dict(torch.load(tmp_path / "opt.pth", weights_only=False))
    _steps(pc, oc, grads[2:], skip=4)
    assert all(torch.equal(a, c) for a, c in zip(pa, pc))
    sa, sc = oa.state_dict(), oc.state_dict()
    assert sorted(sa["state"]) == sorted(sc["state"]) == [0, 1, 2, 3]
    for i in sa["state"]:
        assert float(sc["state"][i]["step"]) == 4.0
        assert all(torch.equal(sa["state"][i][k], sc["state"][i][k]) for k in ("exp_avg", "exp_avg_sq"))
    assert torch.equal(pa[4].detach().cpu(), init[4])
    # ... and the same file under torch.optim.Adam
    pt = [torch.nn.Parameter(p.detach().clone()) for p in pb]
    ot = torch.optim.Adam([{"params": pt[:2], "lr": 1e-3}, {"params": pt[2:], "lr": 1e-2}], weight_decay=0.01)
    ot.load_state_dict(torch.load(tmp_path / "opt.pth", weights_only=False))
    st = ot.state_dict()["state"]
    assert sorted(st) == [0, 1, 2, 3] and all(float(st[i]["step"]) == 2.0 for i in st)


def test_step_refuses_graph_capture(monkeypatch):
    """(the stream is only SAID to be capturing: what is checked is that step() asks, and touches nothing then)"""
    dev = torch.device("cuda:0")
    init, grads = _recorded([(8,), (8,)], 1, 2)
    params, opt = _make(init, dev)
    _steps(params, opt, grads)
    torch.cuda.synchronize()
    before = [p.detach().clone() for p in params]
    steps = opt._steps.copy()
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(RuntimeError, match="cannot be captured"):
        opt.step()
    monkeypatch.undo()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(before, params)) and np.array_equal(steps, opt._steps)


def _fp64_adam(p, grads, lr, wd, betas=(0.9, 0.999), eps=1e-8):
    p = p.double()
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    for step, g in enumerate(grads, 1):
        g = g.double() + wd * p
        m = betas[0] * m + (1 - betas[0]) * g
        v = betas[1] * v + (1 - betas[1]) * g * g
        p = p - lr / (1 - betas[0] ** step) * m / (v.sqrt() / (1 - betas[1] ** step) ** 0.5 + eps)
    return p


def test_agreement_with_torch_on_both_nets():
    """DispResNet(18)'s and PoseResNet(18)'s parameter lists, generated gradients, five steps.  The yardstick is
    torch.optim.Adam(foreach=False) on the device against an fp64 Adam on the host: per tensor, this optimiser's worst
    error may be at most twice torch's own plus ULPS ulp of the tensor's largest parameter."""
    import models
    from scsfm_hip import optim
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    nets = [models.DispResNet(18, False), models.PoseResNet(18, False)]
    shapes = [tuple(p.shape) for net in nets for p in net.parameters()]
    init = [p.detach().clone() for net in nets for p in net.parameters()]
    g = torch.Generator().manual_seed(5)
    grads = [[torch.randn(s, generator=g) * 10.0 ** float(torch.randint(-4, 1, (1,), generator=g)) for s in shapes]
             for _ in range(5)]
    lr, wd = 1e-4, 0.0
    n0 = len(list(nets[0].parameters()))
    results = {}
    for name, cls, kw in (("torch", torch.optim.Adam, dict(foreach=False)), ("hip", optim.Adam, {})):
        params = [torch.nn.Parameter(t.to(dev)) for t in init]
        opt = cls([{"params": params[:n0], "lr": lr}, {"params": params[n0:], "lr": lr}], betas=(0.9, 0.999),
                  weight_decay=wd, **kw)
        _steps(params, opt, grads)
        torch.cuda.synchronize()
        results[name] = [p.detach().cpu() for p in params]
    worst, need = 0.0, 0.0
    for k, (p0, t, h) in enumerate(zip(init, results["torch"], results["hip"])):
        want = _fp64_adam(p0, [gs[k] for gs in grads], lr, wd)
        err_t, err_h = float((t.double() - want).abs().max()), float((h.double() - want).abs().max())
        ulp = 2.0 ** -23 * float(want.abs().max())
        ratio = err_h / max(err_t, ulp / 2)
        worst = max(worst, ratio)
        need = max(need, (err_h - 2 * err_t) / ulp)
        assert err_h <= 2 * err_t + ULPS * ulp, (k, shapes[k], err_h, err_t, ulp)
    print(f"worst ratio of this optimiser's error to torch's own over {len(shapes)} tensors: {worst:.3f}; "
          f"ulp of the parameter needed on top of twice torch's error: {need:.3f}")
