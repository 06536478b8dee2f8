"""The validation kernels (csrc_val/*.hip, compiled unchanged against the host simulator) against the numpy oracle
(tests/validation_errors_oracle.py): medians bit for bit (and equal to torch.median on the CPU), the valid count and the
three thresholds' counts exactly, the three means to 1e-12 of the float64 sums, the fused 1 / disp and nearest resize
equal to F.interpolate's, every planted edge case, determinism, and nothing written outside the outputs."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _hostsim_val as S
import _validation_errors_cases as C
import validation_errors_oracle as O


@pytest.mark.parametrize("name", sorted(C.CASES))
def test_case_against_the_oracle(name):
    gt, disp, dataset = C.CASES[name]()
    want = C.expected(name)
    got = S.depth_errors(gt, disp, dataset, is_disp=True)
    C.check(got, want)
    if name == "A":
        assert want[0]["n"] % 2 == 1 and want[1]["n"] % 2 == 0
        g = np.sort(gt[2][15:36, 4:119][gt[2][15:36, 4:119] > 0])
        assert g[(g.size - 1) // 2] == g[(g.size - 1) // 2 + 1]  # image (c): the middle ranks are a tie
    if name == "C":
        assert want[0]["n"] > 65536
    # the medians are torch.median's, of the gathers the reference makes
    depth = F.interpolate((1 / torch.tensor(disp)).unsqueeze(1), list(gt.shape[1:])).squeeze(1)
    y1, y2, x1, x2, cap = O.crop_and_cap(dataset, *gt.shape[1:])
    for i, (g, p) in enumerate(zip(torch.tensor(gt), depth)):
        valid = (g > 0.1) & (g < float(cap))
        box = torch.zeros_like(valid)
        box[y1:y2, x1:x2] = True
        valid &= box
        med = [torch.median(g[valid]).item(), torch.median(p[valid].clamp(1e-3, float(cap))).item()]
        assert C.same_bits(got["medians"][i], np.array(med, np.float32))
        assert got["count"][i] == int(valid.sum())


@pytest.mark.parametrize("name", ("A", "B"))
def test_fused_inverse_and_resize_equal_interpolate(name):
    """1 / disp and F.interpolate(., [H, W]) on the CPU, fed to the library and to the oracle as a depth of the ground
    truth's size, give what the library makes of the disparity itself."""
    gt, disp, dataset = C.CASES[name]()
    depth = F.interpolate((1 / torch.tensor(disp)).unsqueeze(1), list(gt.shape[1:])).squeeze(1).numpy()
    fused = S.depth_errors(gt, disp, dataset, is_disp=True)
    plain = S.depth_errors(gt, depth, dataset, is_disp=False)
    for k in fused:
        assert C.same_bits(fused[k], plain[k]), k
    C.check(fused, O.depth_errors(gt, depth, dataset))


@pytest.mark.parametrize("kind", C.EDGES)
def test_edge_cases(kind):
    gt, src, dataset = C.edge(kind)
    want = O.depth_errors(gt, src, dataset)
    got = S.depth_errors(gt, src, dataset)
    C.check(got, want)
    row, n = got["metrics"][1], got["count"][1]
    if kind == "empty":
        assert n == 0 and np.isnan(row).all() and np.isnan(got["medians"][1]).all()
    elif kind == "one_pixel":
        assert n == 1 and got["medians"][1, 0] == np.float32(12.5) and row[0] == 0 and (row[3:] == 1).all()
    elif kind == "all_equal":
        assert got["medians"][1, 0] == np.float32(7.25)
    elif kind == "nan_pred":
        assert n > 0 and np.isnan(row).all() and np.isnan(got["medians"][1, 1]) and got["medians"][1, 0] > 0
    else:
        assert n > 0 and np.isfinite(row).all()
    if kind == "nan_gt":
        g0 = C.case_a()[0][1]
        lost = sum(0.1 < g0[r, c] < 80 for r, c in ((17, 6), (19, 13)))  # where the NaN and the infinity were planted
        assert lost >= 1 and n == C.expected("A")[1]["n"] - lost  # they left the mask, nothing else did
    if kind == "clamp":
        plain = O.depth_errors(gt, np.clip(src, 1e-3, 80).astype(np.float32), dataset)
        assert C.same_bits(want[1]["metrics"], plain[1]["metrics"])
    # the other images of the batch are unaffected by what was planted into image 1
    base = S.depth_errors(C.case_a()[0], src, dataset)
    for k in got:
        assert C.same_bits(got[k][[0, 2]], base[k][[0, 2]]), k


def test_batch_split_and_rerun_are_bit_identical():
    gt, disp, dataset = C.case_a()
    whole = S.depth_errors(gt, disp, dataset, is_disp=True)
    again = S.depth_errors(gt, disp, dataset, is_disp=True)
    # one image per call, from a buffer shifted by one element (off the 16-byte boundary: the element-wise loads)
    shifted = np.zeros(gt.size + 1, np.float32)[1:].reshape(gt.shape)
    shifted[...] = gt
    for k in whole:
        assert C.same_bits(whole[k], again[k]), k
        parts = np.concatenate([S.depth_errors(gt[i:i + 1], disp[i:i + 1], dataset, is_disp=True)[k] for i in range(3)])
        assert C.same_bits(whole[k], parts), k
        moved = np.concatenate([S.depth_errors(shifted[i:i + 1], disp[i:i + 1], dataset, is_disp=True)[k]
                                for i in range(3)])
        assert C.same_bits(whole[k], moved), k


def test_rejected_arguments_return_minus_one_and_write_nothing():
    gt, disp, dataset = C.case_a()
    gt, disp = np.ascontiguousarray(gt), np.ascontiguousarray(disp)
    B, H, W = gt.shape
    h, w = disp.shape[1:]
    L = S.lib()
    nbytes = L.size("scsfm_val_workspace_bytes", B, H, W)
    assert nbytes > 0
    for bad in ((0, H, W), (B, 0, W), (B, H, -1), (1 << 15, 1 << 8, 1 << 8)):
        assert L.size("scsfm_val_workspace_bytes", *bad) == 0
    ws = np.full(nbytes, 0xAB, np.uint8)
    box = O.crop_and_cap(dataset, H, W)[:4]
    ok = dict(B=B, h=h, w=w, src=disp, is_disp=1, H=H, W=W, gt=gt, box=box, min_gt=0.1, max_depth=80.0, clamp_lo=1e-3,
              ws=ws, ws_bytes=nbytes)
    bad = [dict(B=0), dict(B=-1), dict(h=0), dict(w=0), dict(H=0), dict(W=-3),
           dict(box=(-1, 36, 4, 119)), dict(box=(15, H + 1, 4, 119)), dict(box=(15, 36, -1, 119)),
           dict(box=(15, 36, 4, W + 1)), dict(box=(36, 15, 4, 119)), dict(box=(15, 36, 119, 4)),
           dict(min_gt=80.0), dict(min_gt=90.0), dict(max_depth=float("nan")), dict(ws_bytes=nbytes - 1),
           dict(null=("src",)), dict(null=("gt",)), dict(null=("ws",)), dict(null=("metrics",)),
           dict(null=("medians",)), dict(null=("count",))]
    for change in bad:
        bufs = S.outputs(B)
        assert S.raw(**dict(ok, **change), bufs=bufs) == -1, change
        assert S.untouched(bufs) and (ws == 0xAB).all(), change
    bufs = S.outputs(B)  # ... and the unchanged arguments are accepted
    assert S.raw(**ok, bufs=bufs) == 0 and S.untouched(bufs, B) and not S.untouched(bufs)


def test_python_layer_on_the_simulator(monkeypatch):
    """scsfm_hip.validation's argument handling: the crop box per dataset, the reference's UnboundLocalError for any
    other name, batch_mean's division and NaN propagation."""
    from scsfm_hip import validation as V
    assert V.crop_and_cap("kitti", 37, 124) == (15, 36, 4, 119, 80)
    assert V.crop_and_cap("nyu", 48, 64) == (4, 47, 4, 60, 10)
    with pytest.raises(UnboundLocalError, match="dataset must be 'kitti' or 'nyu', got 'cityscapes'"):
        V.depth_errors(torch.zeros(1, 4, 4), torch.zeros(1, 4, 4), "cityscapes")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        V.depth_errors(torch.zeros(1, 4, 4), torch.zeros(1, 4, 4), "kitti")
    with pytest.raises(TypeError):
        V.depth_errors(torch.zeros(1, 4, 4, dtype=torch.float64), torch.zeros(1, 4, 4), "kitti")
    m = torch.tensor([[1.0, 2, 3, 4, 5, 6], [3.0, 2, float("nan"), 0, 1, 2]], dtype=torch.float64)
    got = V.batch_mean(V.DepthErrors(m, None, None))
    assert got[:2] == [2.0, 2.0] and np.isnan(got[2]) and got[3:] == [2.0, 3.0, 4.0]


def test_compute_errors_keeps_the_torch_body_for_cpu_tensors(golden_dir):
    """CPU tensors and other dtypes never reach the library: compute_errors' torch body gives the goldens."""
    import loss_functions as LF
    gold = np.load(f"{golden_dir}/misc.npz")
    for ds in ("kitti", "nyu"):
        gt, pred = torch.from_numpy(gold[f"errors/{ds}/gt"]), torch.from_numpy(gold[f"errors/{ds}/pred"])
        np.testing.assert_allclose(LF.compute_errors(gt, pred, ds), gold[f"errors/{ds}/out"], rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(LF.compute_errors(gt.double(), pred.double(), ds), gold[f"errors/{ds}/out"],
                                   rtol=1e-5, atol=1e-6)
    with pytest.raises(UnboundLocalError, match="dataset must be 'kitti' or 'nyu'"):
        LF.compute_errors(torch.zeros(1, 4, 4), torch.zeros(1, 4, 4), "cityscapes")
