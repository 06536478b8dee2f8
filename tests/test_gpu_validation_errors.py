"""libscsfm_val.so on the device, through scsfm_hip.validation: the cases and edge cases of the host-simulator tests
against the same numpy oracle with the same exactness claims, medians and counts bit-equal to torch's on the GPU,
compute_errors' dispatch against its torch body and the goldens, and one validate_with_gt run against the sequence it
replaces (1 / disp, F.interpolate, the torch body)."""
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _validation_errors_cases as C
import validation_errors_oracle as O

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")


def run(gt, src, dataset, is_disp=False):
    from scsfm_hip import validation as V
    res = V.depth_errors(torch.tensor(gt).to(DEV), torch.tensor(src).to(DEV), dataset, is_disp=is_disp)
    assert res.metrics.device.type == "cuda" and res.medians.device.type == "cuda" and res.count.device.type == "cuda"
    return dict(metrics=res.metrics.cpu().numpy(), medians=res.medians.cpu().numpy(), count=res.count.cpu().numpy())


@pytest.fixture
def torch_body():
    """Forces compute_errors' torch body for the duration of a with-block."""
    from scsfm_hip import config

    class Switch:
        def __enter__(self):
            config.set_errors_on_torch(True)

        def __exit__(self, *exc):
            config.set_errors_on_torch(False)

    yield Switch()
    config.set_errors_on_torch(False)


@pytest.mark.parametrize("name", sorted(C.CASES))
def test_case_against_the_oracle_and_torch(name):
    gt, disp, dataset = C.CASES[name]()
    got = run(gt, disp, dataset, is_disp=True)
    C.check(got, C.expected(name))
    again = run(gt, disp, dataset, is_disp=True)
    for k in got:
        assert C.same_bits(got[k], again[k]), k
    # torch on the GPU: the gathers the reference makes, its medians and its counts (of the correctly rounded 1 / disp)
    g_all = torch.tensor(gt).to(DEV)
    depth = F.interpolate((1 / torch.tensor(disp)).unsqueeze(1), list(gt.shape[1:])).squeeze(1).to(DEV)
    y1, y2, x1, x2, cap = O.crop_and_cap(dataset, *gt.shape[1:])
    box = torch.zeros(gt.shape[1:], dtype=torch.bool, device=DEV)
    box[y1:y2, x1:x2] = True
    for i, (g, p) in enumerate(zip(g_all, depth)):
        valid = (g > 0.1) & (g < float(cap)) & box
        med = [torch.median(g[valid]).item(), torch.median(p[valid].clamp(1e-3, float(cap))).item()]
        assert C.same_bits(got["medians"][i], np.array(med, np.float32))
        assert got["count"][i] == int(valid.sum())
    if name == "A":  # a batch of three is three batches of one
        for k in got:
            parts = np.concatenate([run(gt[i:i + 1], disp[i:i + 1], dataset, is_disp=True)[k] for i in range(3)])
            assert C.same_bits(got[k], parts), k


@pytest.mark.parametrize("kind", C.EDGES)
def test_edge_cases(kind):
    gt, src, dataset = C.edge(kind)
    got = run(gt, src, dataset)
    C.check(got, O.depth_errors(gt, src, dataset))
    if kind in ("empty", "nan_pred"):
        assert np.isnan(got["metrics"][1]).all() and np.isfinite(got["metrics"][[0, 2]]).all()
        from scsfm_hip import validation as V
        mean = V.batch_mean(V.DepthErrors(torch.tensor(got["metrics"]), None, None))
        assert np.isnan(mean).all()


@pytest.mark.parametrize("name", sorted(C.CASES))
def test_compute_errors_dispatch_against_the_torch_body(name, torch_body, monkeypatch):
    import loss_functions as LF
    from scsfm_hip import validation as V
    gt, disp, dataset = C.CASES[name]()
    g = torch.tensor(gt).to(DEV)
    depth = F.interpolate((1 / torch.tensor(disp).to(DEV)).unsqueeze(1), list(gt.shape[1:])).squeeze(1)
    calls = []
    real = V.depth_errors
    monkeypatch.setattr(V, "depth_errors", lambda *a, **k: calls.append(1) or real(*a, **k))
    with torch_body:
        want = LF.compute_errors(g, depth, dataset)
    assert not calls
    got = LF.compute_errors(g, depth, dataset)
    assert len(calls) == 1  # the library, once per batch
    assert isinstance(got, list) and len(got) == 6 and all(isinstance(v, float) for v in got)
    np.testing.assert_allclose(got, want, rtol=1e-5, atol=0)
    np.testing.assert_allclose(got, O.batch_mean(C.expected(name)), rtol=1e-12, atol=0)
    # other dtypes keep the torch body
    LF.compute_errors(g.double(), depth.double(), dataset)
    assert len(calls) == 1
    with pytest.raises(UnboundLocalError, match="dataset must be 'kitti' or 'nyu', got 'cityscapes'"):
        LF.compute_errors(g, depth, "cityscapes")


@pytest.mark.parametrize("dataset", ("kitti", "nyu"))
def test_compute_errors_on_the_goldens(dataset, golden_dir):
    import loss_functions as LF
    gold = np.load(f"{golden_dir}/misc.npz")
    out = LF.compute_errors(torch.from_numpy(gold[f"errors/{dataset}/gt"]).to(DEV),
                            torch.from_numpy(gold[f"errors/{dataset}/pred"]).to(DEV), dataset)
    np.testing.assert_allclose(out, gold[f"errors/{dataset}/out"], rtol=1e-5, atol=1e-6)


def test_validate_with_gt_equals_the_sequence_it_replaces(torch_body):
    """A tiny DispResNet18 on two batches of 2 x 3 x 64 x 224 against ground truth of 37 x 124: the returned averages
    against 1 / disp, F.interpolate and the torch body on the same network outputs.  (64 x 224, not 64 x 208: the
    network takes sizes that are multiples of 32 only -- at 208 columns its decoder's skip connections do not line up,
    here as in the reference.)"""
    import loss_functions as LF
    import models
    import train as T
    from logger import AverageMeter
    torch.manual_seed(5)
    inner = models.DispResNet(18, False).to(DEV)

    class Recording(torch.nn.Module):  # (the comparison below runs on the very outputs validate_with_gt saw)
        def __init__(self):
            super().__init__()
            self.net, self.outs = inner, []

        def forward(self, x):
            self.outs.append(self.net(x))
            return self.outs[-1]

    net = Recording()
    rng = np.random.default_rng(21)
    loader = []
    for _ in range(2):
        gt = rng.uniform(0.05, 90.0, (2, 37, 124)).astype(np.float32)
        gt[rng.random(gt.shape) < 0.5] = 0
        loader.append((torch.randn(2, 3, 64, 224), torch.tensor(gt)))
    lines = []
    logger = types.SimpleNamespace(valid_bar=types.SimpleNamespace(update=lambda i: None),
                                   valid_writer=types.SimpleNamespace(write=lines.append))
    args = types.SimpleNamespace(dataset="kitti", print_freq=1)
    T.device = DEV
    got, names = T.validate_with_gt(args, loader, net, 0, logger)
    assert names == ['abs_diff', 'abs_rel', 'sq_rel', 'a1', 'a2', 'a3'] and len(got) == 6
    assert len(lines) == 2 and lines[0].startswith("valid: Time ") and " Abs Error " in lines[0]

    want = AverageMeter(i=6)
    assert len(net.outs) == 2 and tuple(net.outs[0].shape) == (2, 1, 64, 224) and not inner.training
    with torch.no_grad(), torch_body:
        for (img, depth), disp in zip(loader, net.outs):
            depth = depth.to(DEV)
            out = 1 / disp[:, 0]
            out = F.interpolate(out.unsqueeze(1), [37, 124]).squeeze(1)
            want.update(LF.compute_errors(depth, out, "kitti"))
    assert np.isfinite(got).all()
    np.testing.assert_allclose(got, want.avg, rtol=1e-5, atol=0)
