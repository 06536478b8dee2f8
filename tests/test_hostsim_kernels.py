"""CPU-only checks of the HIP kernels' logic: the product sources compiled unchanged against
tests/hostsim (fibers instead of GPU threads) and compared with the oracle and the goldens recorded
from the reference.  fp64 instantiations pin the formulas (1e-10); fp32 is what ships."""
import itertools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from _util import assert_close_frac, leaf, load_inputs, load_npz
from hostsim import harness
from oracle import scsfm_oracle as O
from scsfm_hip import capi, synth
from scsfm_hip._lib import ScsfmError

# Pose gradients are sums dominated by a few near pixels (depth spans 0.1 .. 100), so one mask decision
# that rounds the other way moves them by ~1 %: the reference's own fp32 result differs from its fp64
# result by up to 1.2 % on such data (tests/test_gpu_parity.py measures this per case).
POSE_RTOL = 1.5e-2
FLAGS = [(1, 1, 1), (1, 1, 0), (1, 0, 1), (1, 0, 0), (0, 1, 1), (0, 1, 0), (0, 0, 1), (0, 0, 0)]


@pytest.fixture(scope="module")
def lib():
    return harness.lib()


def _pair_inputs(d, dtype, pose_scale=1.0):
    c = lambda x: x.to(dtype).contiguous()
    return [c(d["tgt_img"]), c(d["ref_imgs"][0]), c(d["tgt_depth"][0]), c(d["ref_depths"][0][0]),
            c(d["poses"][0] * pose_scale), c(d["intrinsics"])]


def _rel(a, b):
    return float((a - b).abs().max() / (b.abs().max() + 1e-300))


@pytest.mark.parametrize("pad", ["zeros", "border"])
@pytest.mark.parametrize("flags3", FLAGS)
def test_pair_fp64_matches_oracle_autograd(lib, flags3, pad):
    d = synth.make_batch(2, 72, 100, n_ref=1, seed=21, depth="smooth")  # ragged: partial tiles on both axes
    ti, ri, td, rd, po, K = _pair_inputs(d, torch.float64)
    ssim, mask, auto = flags3
    fl = capi.make_flags(ssim, mask, auto, pad)
    out, ws = capi.pair_fwd(lib, ti, ri, td, rd, po, K, fl)
    tdl, rdl, pol = leaf(td), leaf(rd), leaf(po)
    diff_img, diff_depth, m = O.pairwise_maps(ti, ri, tdl, rdl, pol, K, ssim, mask, auto, pad)
    # compare the raw sums (independent of the 10000-pixel gate) ...
    assert abs(float(out[4]) - float(m.sum())) == 0
    assert abs(float(out[2]) - float((diff_img * m).sum().detach())) < 1e-9
    assert abs(float(out[3]) - float((diff_depth * m).sum().detach())) < 1e-9
    # ... and the gradients of the un-gated means
    Sm = m.sum()
    L = 0.7 * (diff_img * m).sum() / (3 * Sm) + 1.3 * (diff_depth * m).sum() / Sm
    L.backward()
    # open the gate for the kernel: scale the upstream gradients instead (linear)
    gate_p = 1.0 if 3 * float(Sm) > 10000 else 0.0
    gate_g = 1.0 if float(Sm) > 10000 else 0.0
    assert gate_p == 1.0  # chosen sizes keep the photo gate open
    gt, gr, gp = capi.pair_bwd(lib, ti, ri, td, rd, po, K, fl, ws, torch.tensor([0.7], dtype=torch.float64),
                               torch.tensor([1.3], dtype=torch.float64))
    if gate_g == 1.0:
        assert _rel(gt, tdl.grad) < 1e-10 and _rel(gr, rdl.grad) < 1e-10 and _rel(gp, pol.grad) < 1e-10
    else:  # geometry gated off: compare against the photo-only gradient
        tdl2, rdl2, pol2 = leaf(td), leaf(rd), leaf(po)
        di, dd, m2 = O.pairwise_maps(ti, ri, tdl2, rdl2, pol2, K, ssim, mask, auto, pad)
        (0.7 * (di * m2).sum() / (3 * m2.sum())).backward()
        assert _rel(gt, tdl2.grad) < 1e-10 and _rel(gp, pol2.grad) < 1e-10


def test_pair_gate_closed_gives_zero_loss_and_zero_gradients(lib):
    d = load_inputs("tiny")  # 2 x 24 x 40 = 1920 pixels: below both gates
    ti, ri, td, rd, po, K = _pair_inputs(d, torch.float32)
    fl = capi.make_flags(1, 1, 0, "zeros")
    out, ws = capi.pair_fwd(lib, ti, ri, td, rd, po, K, fl)
    assert float(out[0]) == 0.0 and float(out[1]) == 0.0 and float(out[4]) > 0
    one = torch.ones(1)
    gt, gr, gp = capi.pair_bwd(lib, ti, ri, td, rd, po, K, fl, ws, one, one)
    assert float(gt.abs().max()) == 0 and float(gr.abs().max()) == 0 and float(gp.abs().max()) == 0
    gold = load_npz("pair_tiny.npz")
    assert float(gold["110_zeros/photo"]) == 0.0 and float(gold["110_zeros/geom"]) == 0.0


@pytest.mark.parametrize("name", ["smooth", "iid"])
def test_pair_fp32_matches_reference_goldens(lib, name):
    d = load_inputs(name)
    gold = load_npz(f"pair_{name}.npz")
    ti, ri, td, rd, po, K = _pair_inputs(d, torch.float32)
    w_photo, w_geom = torch.tensor([1.0]), torch.tensor([0.5])
    for (ssim, mask, auto), pad in itertools.product(FLAGS, ("zeros", "border")):
        key = f"{ssim}{mask}{auto}_{pad}"
        fl = capi.make_flags(ssim, mask, auto, pad)
        out, ws = capi.pair_fwd(lib, ti, ri, td, rd, po, K, fl)
        # the parity bar of the path: 1e-5 absolute on the fp32 losses
        assert abs(float(out[0]) - float(gold[f"{key}/photo"])) <= 1e-5, key
        assert abs(float(out[1]) - float(gold[f"{key}/geom"])) <= 1e-5, key
        gt, gr, gp = capi.pair_bwd(lib, ti, ri, td, rd, po, K, fl, ws, w_photo, w_geom)
        g_pose = gold[f"{key}/g_pose"]
        assert_close_frac(gp.numpy(), g_pose, atol=POSE_RTOL * np.abs(g_pose).max() + 1e-7, what=key + " g_pose")
        for nm, g in (("g_tgt_depth", gt), ("g_ref_depth", gr)):
            st = gold[f"{key}/{nm}_stats"]
            f = g.double().reshape(-1)
            assert abs(float(f.abs().sum()) - st[1]) <= 2e-3 * st[1] + 1e-9, (key, nm)
            if f"{key}/{nm}" in gold:
                ref = gold[f"{key}/{nm}"]
                # discontinuous gates may flip isolated pixels: bound their share
                assert_close_frac(g.numpy(), ref, atol=2e-3 * np.abs(ref).max(), rtol=1e-3, max_bad_frac=2e-3,
                                  what=f"{key} {nm}")


@pytest.mark.parametrize("name", ["smooth", "iid"])
def test_warp_maps_match_reference_goldens(lib, name):
    d = load_inputs(name)
    gold = load_npz(f"maps_{name}.npz")
    ti, ri, td, rd, po, K = _pair_inputs(d, torch.float32)
    for pad in ("zeros", "border"):
        w, v, pd, cd = capi.warp_fwd(lib, ri, td, rd, po, K, capi.make_flags(padding_mode=pad))
        assert (v.numpy().astype(np.uint8) != gold[f"{pad}/valid_mask"]).mean() <= 1e-3
        # iid images have unit-scale differences between neighbours, so a 1e-4 px coordinate rounding
        # difference shows up at the 1e-4 level in the sampled colours
        assert_close_frac(w.numpy(), gold[f"{pad}/projected_img"], atol=3e-4, max_bad_frac=1e-3, what="img")
        # same for the sampled depth (iid depth jumps by up to 100 between neighbours)
        pd_atol = 1e-5 if name == "smooth" else 1e-4 * float(np.abs(gold[f"{pad}/projected_depth"]).max())
        assert_close_frac(pd.numpy(), gold[f"{pad}/projected_depth"], atol=pd_atol, rtol=2e-5, max_bad_frac=1e-3,
                          what="pdepth")
        assert_close_frac(cd.numpy(), gold[f"{pad}/computed_depth"], atol=1e-5, rtol=1e-5, what="cdepth")


@pytest.mark.parametrize("pad", ["zeros", "border"])
def test_warp_backward_fp64(lib, pad):
    d = synth.make_batch(2, 40, 72, n_ref=1, seed=5)
    ti, ri, td, rd, po, K = _pair_inputs(d, torch.float64, pose_scale=3.0)
    g = torch.Generator().manual_seed(1)
    gi, gpd, gcd = (torch.randn(s, generator=g, dtype=torch.float64) for s in (ri.shape, td.shape, td.shape))
    tdl, rdl, pol = leaf(td), leaf(rd), leaf(po)
    ow, ov, opd, ocd = O.inverse_warp2(ri, tdl, rdl, pol, K, pad)
    ((ow * gi).sum() + (opd * gpd).sum() + (ocd * gcd).sum()).backward()
    gd, gr, gp = capi.warp_bwd(lib, ri, td, rd, po, K, capi.make_flags(padding_mode=pad), gi, gpd, gcd)
    assert _rel(gd, tdl.grad) < 1e-10 and _rel(gr, rdl.grad) < 1e-10 and _rel(gp, pol.grad) < 1e-10
    # missing upstream maps are skipped, not read
    gd2, gr2, gp2 = capi.warp_bwd(lib, ri, td, rd, po, K, capi.make_flags(padding_mode=pad), gi, None, None)
    tdl, rdl, pol = leaf(td), leaf(rd), leaf(po)
    ow, _, _, _ = O.inverse_warp2(ri, tdl, rdl, pol, K, pad)
    (ow * gi).sum().backward()
    assert _rel(gd2, tdl.grad) < 1e-10 and float(gr2.abs().max()) == 0 and _rel(gp2, pol.grad) < 1e-10


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("name", ["smooth", "iid"])
def test_total_loss_fp32_matches_reference_goldens(lib, name, fused):
    """compute_photo_and_geometry_loss + compute_smooth_loss over 2 refs, 1 and 2 scales, through the
    same capi pipeline the autograd node uses.  ``fused``: the coarser scale's maps go to the library as they are
    (scsfm_pair_desc::depth_shift) instead of being up-sampled with F.interpolate first."""
    d = load_inputs(name)
    gold = load_npz(f"total_{name}.npz")
    H, W = d["tgt_img"].shape[-2:]
    for n_scales in (1, 2):
        for ssim, mask, auto, pad in ((1, 1, 1, "zeros"), (1, 1, 0, "border")):
            key = f"s{n_scales}_{ssim}{mask}{auto}_{pad}"
            td = [leaf(x) for x in d["tgt_depth"]]
            rd = [[leaf(x) for x in r] for r in d["ref_depths"]]
            up = lambda t, s: t if s == 0 or fused else F.interpolate(t, (H, W), mode="nearest")
            td_full = [up(td[s], s) for s in range(n_scales)]
            rd_full = [[up(r[s], s) for s in range(n_scales)] for r in rd]
            det = lambda ts: [t.detach().contiguous() for t in ts]
            fl = capi.make_flags(ssim, mask, auto, pad)
            photo, geom, outs, wss = capi.photo_geometry_fwd(lib, fl, d["tgt_img"], d["intrinsics"], d["ref_imgs"],
                                                             det(td_full), [det(r) for r in rd_full], d["poses"],
                                                             d["poses_inv"])
            smooth, sws = capi.smooth_multi_fwd(lib, [td[0].detach()] + [r[0].detach() for r in rd],
                                                [d["tgt_img"]] + d["ref_imgs"])
            assert abs(float(photo) - float(gold[f"{key}/photo"])) <= 1e-5
            assert abs(float(geom) - float(gold[f"{key}/geom"])) <= 1e-5
            assert abs(float(smooth) - float(gold[f"{key}/smooth"])) <= 1e-5
            g_td, g_rd, g_p, g_pi = capi.photo_geometry_bwd(lib, fl, d["tgt_img"], d["intrinsics"], d["ref_imgs"],
                                                            det(td_full), [det(r) for r in rd_full], d["poses"],
                                                            d["poses_inv"], wss, torch.tensor([1.0]),
                                                            torch.tensor([0.5]))
            # chain through the nearest up-sampling (autograd, as loss_functions.py does) and add smooth
            for s in range(n_scales):
                assert g_td[s].shape == td_full[s].shape
                td_full[s].backward(g_td[s]) if s > 0 else None  # (fused: td_full[s] IS the leaf)
                for i in range(2):
                    rd_full[i][s].backward(g_rd[i][s]) if s > 0 else None
            frames = [td[0]] + [r[0] for r in rd]
            g_sm = capi.smooth_multi_bwd(lib, [f.detach() for f in frames], [d["tgt_img"]] + d["ref_imgs"], sws,
                                         torch.tensor([0.1]))
            tot_t0 = g_td[0] + g_sm[0]
            ref = gold[f"{key}/g_tgt_depth_s0"]
            assert_close_frac(tot_t0.numpy(), ref, atol=2e-3 * np.abs(ref).max(), rtol=1e-3, max_bad_frac=2e-3,
                              what=key + " tgt s0")
            for i in range(2):
                ref = gold[f"{key}/g_ref{i}_depth_s0"]
                assert_close_frac((g_rd[i][0] + g_sm[1 + i]).numpy(), ref, atol=2e-3 * np.abs(ref).max(), rtol=1e-3,
                                  max_bad_frac=2e-3, what=f"{key} ref{i} s0")
                assert_close_frac(g_p[i].numpy(), gold[f"{key}/g_pose{i}"], atol=POSE_RTOL * np.abs(gold[f"{key}/g_pose{i}"]).max())
                assert_close_frac(g_pi[i].numpy(), gold[f"{key}/g_pose_inv{i}"],
                                  atol=POSE_RTOL * np.abs(gold[f"{key}/g_pose_inv{i}"]).max())
            if n_scales == 2:
                ref = gold[f"{key}/g_tgt_depth_s1"]
                assert_close_frac(td[1].grad.numpy(), ref, atol=2e-3 * np.abs(ref).max(), rtol=1e-3, max_bad_frac=2e-3)


def test_smooth_matches_oracle_and_golden(lib):
    for dt, tol in ((torch.float64, 1e-12), (torch.float32, 2e-6)):
        for B, H, W in ((2, 80, 112), (3, 37, 131), (1, 2, 2)):
            d = synth.make_batch(B, H, W, n_ref=1, seed=5, depth="iid")
            dep, img = d["tgt_depth"][0].to(dt), d["tgt_img"].to(dt)
            out, ws = capi.smooth_fwd(lib, dep, img)
            dl = leaf(dep)
            L = O.smooth_term(dl, img)
            (2.5 * L).backward()
            g = capi.smooth_bwd(lib, dep, img, ws, torch.tensor([2.5], dtype=dt))
            assert abs(float(out) - float(L)) <= tol * max(1.0, abs(float(L)))
            assert _rel(g, dl.grad) <= (1e-10 if dt == torch.float64 else 1e-5)
    d = load_inputs("smooth")
    gold = load_npz("total_smooth.npz")
    frames = [d["tgt_depth"][0]] + [r[0] for r in d["ref_depths"]]
    imgs = [d["tgt_img"]] + d["ref_imgs"]
    loss, wss = capi.smooth_multi_fwd(lib, frames, imgs)
    assert abs(float(loss) - float(gold["smooth_only/loss"])) <= 1e-5
    g0, g1, g2 = capi.smooth_multi_bwd(lib, frames, imgs, wss, torch.ones(1), need=[True, False, True])
    assert g1 is None and g2 is not None
    assert_close_frac(g0.numpy(), gold["smooth_only/g_tgt_depth"], atol=1e-5 * np.abs(gold["smooth_only/g_tgt_depth"]).max(),
                      rtol=1e-4)


def test_pose_vec2mat_matches_golden(lib):
    gold = load_npz("misc.npz")
    vec = torch.from_numpy(gold["pose/vec"])
    r = torch.from_numpy(gold["pose/probe"])
    for mode in ("euler", "quat"):
        M = capi.pose_fwd(lib, vec, mode)
        np.testing.assert_allclose(M.numpy(), gold[f"pose/{mode}/mat"], atol=1e-6)
        g = capi.pose_bwd(lib, vec, mode, r)
        np.testing.assert_allclose(g.numpy(), gold[f"pose/{mode}/g_vec"], atol=3e-6)
        v64 = vec.double()
        vl = leaf(v64)
        (O.pose_vec2mat(vl, mode) * r.double()).sum().backward()
        assert _rel(capi.pose_bwd(lib, v64, mode, r.double()), vl.grad) < 1e-12


def test_ssim_and_masked_mean_helpers(lib):
    g = torch.Generator().manual_seed(0)
    for dt, tol in ((torch.float64, 1e-11), (torch.float32, 3e-5)):
        for shp in ((2, 3, 40, 72), (1, 1, 2, 2), (2, 2, 17, 130)):
            x = torch.rand(shp, generator=g, dtype=dt)
            y = (x + 0.3 * torch.rand(shp, generator=g, dtype=dt)).contiguous()
            out = capi.ssim_fwd(lib, x, y)
            xl, yl = leaf(x), leaf(y)
            o = O.ssim_map(xl, yl)
            go = torch.rand(shp, generator=g, dtype=dt)
            (o * go).sum().backward()
            gx, gy = capi.ssim_bwd(lib, x, y, go)
            assert float((out - o).abs().max()) <= tol
            assert _rel(gx, xl.grad) <= tol * 10 and _rel(gy, yl.grad) <= tol * 10
        for shp, mshp in (((2, 3, 80, 112), (2, 1, 80, 112)), ((2, 3, 80, 112), (2, 3, 80, 112)),
                          ((2, 1, 30, 40), (2, 1, 30, 40))):
            diff = torch.rand(shp, generator=g, dtype=dt)
            mask = (torch.rand(mshp, generator=g, dtype=dt) > 0.3).to(dt)
            out, ws = capi.masked_mean_fwd(lib, diff, mask)
            dl = leaf(diff)
            o = O.mean_on_mask(dl, mask)
            gd = capi.masked_mean_bwd(lib, shp, mask, ws, torch.tensor([1.7], dtype=dt))
            assert abs(float(out) - float(o)) <= 1e-6
            if o.requires_grad:
                (1.7 * o).backward()
                assert _rel(gd, dl.grad) <= 1e-6
            else:
                assert float(gd.abs().max()) == 0


def test_rejected_arguments_raise(lib):
    d = synth.make_batch(1, 8, 8, n_ref=1, seed=0)
    ti, ri, td, rd, po, K = _pair_inputs(d, torch.float32)
    with pytest.raises(AssertionError, match="wrong size for ref_depth"):
        capi.pair_fwd(lib, ti, ri, td, rd[:, :, :4], po, K, 0)
    with pytest.raises(ScsfmError, match="status -1"):
        capi.smooth_fwd(lib, td[:, :, :1].contiguous(), ti[:, :, :1].contiguous())  # H = 1 < 2
    with pytest.raises(TypeError):
        capi.pair_fwd(lib, ti, ri, td.double(), rd, po, K, 0)
    with pytest.raises(ValueError):
        capi.make_flags(padding_mode="reflection")


@pytest.mark.parametrize("hint,upstream", [((0.7, 1.3), (0.7, 1.3)),   # speculation holds
                                           ((1.0, 0.5), (2.0, 1.0)),   # same ratio, different scale: holds
                                           ((0.7, 1.3), (1.0, 0.5)),   # wrong hint: device-side fallback
                                           (None, (0.7, 1.3))])        # plain forward
def test_speculative_forward_fp64(lib, hint, upstream):
    """scsfm_pair_fwd_spec: the backward's tiled pass run as the forward.  Whatever the hint, losses
    and gradients must equal the oracle's."""
    d = synth.make_batch(2, 72, 100, n_ref=2, seed=23, depth="smooth")
    c = lambda x: x.double().contiguous()
    ti, K = c(d["tgt_img"]), c(d["intrinsics"])
    ris = [c(r) for r in d["ref_imgs"]]
    tds, rds = [c(d["tgt_depth"][0])], [[c(r[0])] for r in d["ref_depths"]]
    ps, pis = [c(p) for p in d["poses"]], [c(p) for p in d["poses_inv"]]
    fl = capi.make_flags(1, 1, 1, "zeros")
    td, rd = [leaf(t) for t in tds], [[leaf(t) for t in r] for r in rds]
    pp, pi = [leaf(p) for p in ps], [leaf(p) for p in pis]
    po, go = O.photo_and_geometry_loss(ti, ris, K, td, rd, pp, pi, 1, 1, 1, 1, "zeros")
    (upstream[0] * po + upstream[1] * go).backward()
    photo, geom, outs, ws = capi.photo_geometry_fwd(lib, fl, ti, K, ris, tds, rds, ps, pis, hint=hint)
    assert abs(float(photo) - float(po)) < 1e-12 and abs(float(geom) - float(go)) < 1e-12
    g_td, g_rd, g_p, g_pi = capi.photo_geometry_bwd(lib, fl, ti, K, ris, tds, rds, ps, pis, ws,
                                                    torch.tensor([upstream[0]], dtype=torch.float64),
                                                    torch.tensor([upstream[1]], dtype=torch.float64))
    z = lambda t: t.grad if t.grad is not None else torch.zeros_like(t)
    assert _rel(g_td[0], z(td[0])) < 1e-10
    for i in range(2):
        assert _rel(g_rd[i][0], z(rd[i][0])) < 1e-10
        assert _rel(g_p[i], z(pp[i])) < 1e-10 and _rel(g_pi[i], z(pi[i])) < 1e-10


def test_repeated_backward_after_a_failed_speculation(lib):
    """retain_graph-style use of one workspace: a backward whose upstream gradients do not stand in the hinted
    ratio (device-side fallback: the speculative planes are overwritten with final values), then one whose
    gradients do.  The second must not rescale the first one's planes."""
    d = synth.make_batch(4, 72, 100, n_ref=1, seed=31, depth="smooth")  # enough pixels to open both gates
    c = lambda x: x.double().contiguous()
    ti, K = c(d["tgt_img"]), c(d["intrinsics"])
    ris = [c(r) for r in d["ref_imgs"]]
    tds, rds = [c(d["tgt_depth"][0])], [[c(r[0])] for r in d["ref_depths"]]
    ps, pis = [c(p) for p in d["poses"]], [c(p) for p in d["poses_inv"]]
    fl = capi.make_flags(1, 1, 1, "zeros")
    _, geom, _, ws = capi.photo_geometry_fwd(lib, fl, ti, K, ris, tds, rds, ps, pis, hint=(1.0, 0.5))
    assert float(geom) > 0  # the geometry gate is open: the upstream ratio matters
    t = lambda v: torch.tensor([v], dtype=torch.float64)
    for up in ((1.0, 0.0), (1.0, 0.5), (0.3, 0.9), (2.0, 1.0)):
        td, rd = [leaf(x) for x in tds], [[leaf(x) for x in r] for r in rds]
        pp, pi = [leaf(p) for p in ps], [leaf(p) for p in pis]
        po, go = O.photo_and_geometry_loss(ti, ris, K, td, rd, pp, pi, 1, 1, 1, 1, "zeros")
        (up[0] * po + up[1] * go).backward()
        g_td, g_rd, g_p, g_pi = capi.photo_geometry_bwd(lib, fl, ti, K, ris, tds, rds, ps, pis, ws, t(up[0]), t(up[1]))
        assert _rel(g_td[0], td[0].grad) < 1e-10, up
        assert _rel(g_rd[0][0], rd[0][0].grad) < 1e-10, up
        assert _rel(g_p[0], pp[0].grad) < 1e-10 and _rel(g_pi[0], pi[0].grad) < 1e-10, up


@pytest.mark.parametrize("hint", [(1.0, 0.5), None])
def test_more_pair_directions_than_one_launch_holds(lib, hint):
    """3 refs x 2 scales x 2 directions = 12 pair-directions > kMaxPairs (8): the library splits them
    over two launches per stage; every gradient buffer still sees every contribution."""
    d = synth.make_batch(2, 64, 96, n_ref=3, seed=29, depth="smooth", num_scales=2)
    c = lambda x: x.double().contiguous()
    H, W = 64, 96
    up = lambda t: F.interpolate(t, (H, W), mode="nearest") if t.shape[-1] != W else t
    ti, K = c(d["tgt_img"]), c(d["intrinsics"])
    ris = [c(r) for r in d["ref_imgs"]]
    tds = [c(up(t)) for t in d["tgt_depth"]]
    rds = [[c(up(t)) for t in r] for r in d["ref_depths"]]
    ps, pis = [c(p) for p in d["poses"]], [c(p) for p in d["poses_inv"]]
    fl = capi.make_flags(1, 1, 0, "zeros")
    td, rd = [leaf(t) for t in tds], [[leaf(t) for t in r] for r in rds]
    pp, pi = [leaf(p) for p in ps], [leaf(p) for p in pis]
    # oracle on the already up-sampled maps: treat each scale as an extra full-resolution pair
    photo_o = geom_o = 0
    for i in range(3):
        for s in range(2):
            a = O.pairwise_loss(ti, ris[i], td[s], rd[i][s], pp[i], K, 1, 1, 0, "zeros")
            b = O.pairwise_loss(ris[i], ti, rd[i][s], td[s], pi[i], K, 1, 1, 0, "zeros")
            photo_o = photo_o + a[0] + b[0]
            geom_o = geom_o + a[1] + b[1]
    (1.0 * photo_o + 0.5 * geom_o).backward()
    photo, geom, outs, ws = capi.photo_geometry_fwd(lib, fl, ti, K, ris, tds, rds, ps, pis, hint=hint)
    assert outs.shape[0] == 12
    assert abs(float(photo) - float(photo_o)) < 1e-11 and abs(float(geom) - float(geom_o)) < 1e-11
    g_td, g_rd, g_p, g_pi = capi.photo_geometry_bwd(lib, fl, ti, K, ris, tds, rds, ps, pis, ws,
                                                    torch.tensor([1.0], dtype=torch.float64),
                                                    torch.tensor([0.5], dtype=torch.float64))
    for s in range(2):
        assert _rel(g_td[s], td[s].grad) < 1e-10
        for i in range(3):
            assert _rel(g_rd[i][s], rd[i][s].grad) < 1e-10
    for i in range(3):
        assert _rel(g_p[i], pp[i].grad) < 1e-10 and _rel(g_pi[i], pi[i].grad) < 1e-10


@pytest.mark.parametrize("pad", ["zeros", "border"])
@pytest.mark.parametrize("hint,upstream", [((1.0, 0.5), (1.0, 0.5)), ((1.0, 0.5), (0.3, 1.1)), (None, (1.0, 0.5))])
def test_four_scales_read_in_place_fp64(lib, hint, upstream, pad):
    """loss_functions.py:77-82 at 4 scales: the coarser maps ([B,1,H>>s,W>>s]) go to the library as they are; the
    kernels read them through the nearest up-sampling's index map and the combining kernel sum-pools the gradients.
    Against the oracle (which up-samples with F.interpolate under autograd) in fp64: speculative forward with a
    holding and a failing hint, and the plain forward + two-pass backward."""
    B, H, W = 2, 80, 104  # multiples of 8; ragged tiles on both axes
    d = synth.make_batch(B, H, W, n_ref=2, seed=57, depth="smooth", num_scales=4)
    c = lambda x: x.double().contiguous()
    ti, K = c(d["tgt_img"]), c(d["intrinsics"])
    ris = [c(r) for r in d["ref_imgs"]]
    tds, rds = [c(t) for t in d["tgt_depth"]], [[c(t) for t in r] for r in d["ref_depths"]]
    assert [tuple(t.shape[-2:]) for t in tds] == [(80, 104), (40, 52), (20, 26), (10, 13)]
    ps, pis = [c(p) for p in d["poses"]], [c(p) for p in d["poses_inv"]]
    td, rd = [leaf(t) for t in tds], [[leaf(t) for t in r] for r in rds]
    pp, pi = [leaf(p) for p in ps], [leaf(p) for p in pis]
    photo_o, geom_o = O.photo_and_geometry_loss(ti, ris, K, td, rd, pp, pi, 4, 1, 1, 1, pad)
    (upstream[0] * photo_o + upstream[1] * geom_o).backward()
    fl = capi.make_flags(1, 1, 1, pad)
    photo, geom, outs, ws = capi.photo_geometry_fwd(lib, fl, ti, K, ris, tds, rds, ps, pis, hint=hint)
    assert outs.shape[0] == 16
    assert abs(float(photo) - float(photo_o)) < 1e-11 and abs(float(geom) - float(geom_o)) < 1e-11
    g_td, g_rd, g_p, g_pi = capi.photo_geometry_bwd(lib, fl, ti, K, ris, tds, rds, ps, pis, ws,
                                                    torch.tensor([upstream[0]], dtype=torch.float64),
                                                    torch.tensor([upstream[1]], dtype=torch.float64))
    for s in range(4):
        assert g_td[s].shape == tds[s].shape
        assert _rel(g_td[s], td[s].grad) < 1e-10, s
        for i in range(2):
            assert _rel(g_rd[i][s], rd[i][s].grad) < 1e-10, (i, s)
    for i in range(2):
        assert _rel(g_p[i], pp[i].grad) < 1e-10 and _rel(g_pi[i], pi[i].grad) < 1e-10


@pytest.mark.parametrize("hint,upstream", [((1.0, 0.5), (1.0, 0.5)), (None, (1.0, 0.5))])
def test_scene_depth_law_fp64(lib, hint, upstream):
    """The `scene` law of round 5 (piecewise-smooth depth, occlusion edges with disparity jumps of tens of pixels,
    image edges on the depth's): the taps of one tile land in two separate places of the reference view, so the
    scatter window / staged taps / direct atomics all carry part of a tile.  fp64 kernels against the oracle."""
    B, H, W = 2, 96, 160
    d = synth.make_batch(B, H, W, n_ref=1, seed=71, depth="scene", image="scene", pose_scale=0.02)
    assert synth.scene_edge_fraction(d["tgt_depth"][0]) > 0.02
    c = lambda x: x.double().contiguous()
    ti, K = c(d["tgt_img"]), c(d["intrinsics"])
    ris = [c(r) for r in d["ref_imgs"]]
    tds, rds = [c(t) for t in d["tgt_depth"]], [[c(t) for t in r] for r in d["ref_depths"]]
    ps, pis = [c(p) for p in d["poses"]], [c(p) for p in d["poses_inv"]]
    td, rd = [leaf(t) for t in tds], [[leaf(t) for t in r] for r in rds]
    pp, pi = [leaf(p) for p in ps], [leaf(p) for p in pis]
    photo_o, geom_o = O.photo_and_geometry_loss(ti, ris, K, td, rd, pp, pi, 1, 1, 1, 1, "zeros")
    (upstream[0] * photo_o + upstream[1] * geom_o).backward()
    fl = capi.make_flags(1, 1, 1, "zeros")
    photo, geom, outs, ws = capi.photo_geometry_fwd(lib, fl, ti, K, ris, tds, rds, ps, pis, hint=hint)
    assert abs(float(photo) - float(photo_o)) < 1e-11 and abs(float(geom) - float(geom_o)) < 1e-11
    g_td, g_rd, g_p, g_pi = capi.photo_geometry_bwd(lib, fl, ti, K, ris, tds, rds, ps, pis, ws,
                                                    torch.tensor([upstream[0]], dtype=torch.float64),
                                                    torch.tensor([upstream[1]], dtype=torch.float64))
    assert _rel(g_td[0], td[0].grad) < 1e-10 and _rel(g_rd[0][0], rd[0][0].grad) < 1e-10
    assert _rel(g_p[0], pp[0].grad) < 1e-10 and _rel(g_pi[0], pi[0].grad) < 1e-10


def test_large_gradients_bypass_the_fixed_point_window(lib):
    """The fp32 speculative forward stages dL/dD_ref in 32-bit fixed-point LDS cells (range +-2048).  Depths just
    above cam2pixel2's 1e-3 clamp and a geometry weight of 5 make the unscaled per-pixel term r * 2Z / (Z + D_p)^2
    ~ 7000: such pixels must take the direct fp32 atomics instead of saturating / wrapping a cell."""
    B, H, W = 2, 72, 100
    d = synth.make_batch(B, H, W, n_ref=1, seed=61, depth="smooth")
    g = torch.Generator().manual_seed(3)
    tds = [1.2e-3 * (1 + 0.05 * torch.rand(B, 1, H, W, generator=g))]
    rds = [[1.0e-3 * (1.02 + 0.05 * torch.rand(B, 1, H, W, generator=g))]]
    p = torch.zeros(B, 6)
    p[:, 0], p[:, 1] = 4e-7, -3e-7  # a fraction of a pixel at this depth: one target pixel per reference pixel, off-grid
    ps, pis = [p], [-p]
    ti, K, ris = d["tgt_img"], d["intrinsics"], d["ref_imgs"]
    c = lambda x: x.double()
    td64, rd64 = [leaf(c(tds[0]))], [[leaf(c(rds[0][0]))]]
    po, go = O.photo_and_geometry_loss(c(ti), [c(ris[0])], c(K), td64, rd64, [c(ps[0])], [c(pis[0])], 1, 1, 1, 0, "zeros")
    (po + 5.0 * go).backward()
    fl = capi.make_flags(1, 1, 0, "zeros")
    photo, geom, outs, ws = capi.photo_geometry_fwd(lib, fl, ti, K, ris, tds, rds, ps, pis, hint=(1.0, 5.0))
    assert abs(float(photo) - float(po)) < 1e-5 and abs(float(geom) - float(go)) < 1e-5
    g_td, g_rd, _, _ = capi.photo_geometry_bwd(lib, fl, ti, K, ris, tds, rds, ps, pis, ws, torch.tensor([1.0]),
                                               torch.tensor([5.0]))
    # the unscaled terms (gradient / the late factor a = g_photo / (3 S_mask)) are beyond a cell's range
    assert float(rd64[0][0].grad.abs().max()) * 3 * float(outs[0, 4]) > 2048
    assert _rel(g_rd[0][0].double(), rd64[0][0].grad) < 1e-3
    assert _rel(g_td[0].double(), td64[0].grad) < 1e-3


@pytest.mark.parametrize("with_mask,up", [(1, (1.0, 1e-4)), (0, (1.0, 1e-4)), (0, (1e-30, 1e-34)), (1, (3e-33, 1e-37))])
def test_fallback_scatter_with_very_different_or_tiny_coefficients_fp32(lib, with_mask, up):
    """The fallback geometry pass (no / failed speculation) stages its scatter in fixed-point cells counted in units of
    the pair's own coefficient.  Round-4 advisor finding: with w_geom << w_photo and no weight mask the scattered
    values are |b|-sized while the unit was max(|a|, |b|) -- 6e-4 of rounding in the median entry, 1.3 % in the worst --,
    and a unit in the subnormal range made 1 / unit infinite.  ONE pair-direction (compute_pairwise_loss), so that
    dL/d ref_depth is the scatter alone; fp32 kernels against the fp64 oracle, entries above 5 % of the map's scale."""
    B, H, W = 4, 72, 100
    d = synth.make_batch(B, H, W, n_ref=1, seed=63, depth="smooth")
    ti, K, ri = d["tgt_img"], d["intrinsics"], d["ref_imgs"][0]
    td, rd, po = d["tgt_depth"][0], d["ref_depths"][0][0], d["poses"][0]
    c = lambda x: x.double()
    td64, rd64 = leaf(c(td)), leaf(c(rd))
    p, g = O.pairwise_loss(c(ti), c(ri), td64, rd64, c(po), c(K), 1, with_mask, 1, "zeros")
    (up[0] * p + up[1] * g).backward()
    fl = capi.make_flags(1, with_mask, 1, "zeros")
    _, ws = capi.pair_fwd(lib, ti, ri, td, rd, po, K, fl)
    _, g_rd, _ = capi.pair_bwd(lib, ti, ri, td, rd, po, K, fl, ws, torch.tensor([up[0]]), torch.tensor([up[1]]))
    want, got = rd64.grad, g_rd.double()
    assert bool(torch.isfinite(got).all())
    big = want.abs() > 0.05 * float(want.abs().max())
    rel = ((got - want).abs() / want.abs())[big]
    assert int(big.sum()) > 1000 and float(rel.median()) < 3e-5 and float(rel.quantile(0.9)) < 1e-4, \
        (float(rel.median()), float(rel.quantile(0.9)))


def _compressive_case(B, scale, tz, seed=67):
    """A scene `scale` times smaller than usual (depths scale * 0.1 .. 0.3) seen after a forward motion of tz * scale:
    every target pixel lands within 5 .. 13 % of its distance from the principal point -- an areal compression of ~100 --
    while the unscaled per-pixel scatter terms 2 Z / (Z + D_p)^2 grow as 1 / scale."""
    H, W = 72, 100
    d = synth.make_batch(B, H, W, n_ref=1, seed=seed, depth="smooth")
    g = torch.Generator().manual_seed(5)
    mk = lambda: (scale * (0.1 + 0.2 * torch.rand(B, 1, H, W, generator=g))).contiguous()
    tds, rds = [mk()], [[mk()]]
    p = torch.zeros(B, 6)
    p[:, 2] = tz * scale
    return d["tgt_img"], d["intrinsics"], d["ref_imgs"], tds, rds, [p], [-p.clone()]


@pytest.mark.parametrize("B,scale,tz,w_geom,hint", [
    (2, 1.0, 1.0, 0.5, (1.0, 0.5)),    # the round-4 review's case: tz = +1, depth 0.1 .. 0.3, 2 x 72 x 100 (geometry gate closed)
    (3, 1.0, 1.0, 0.5, (1.0, 0.5)),    # ... with both gates open
    (3, 0.03, 2.0, 0.0, (1.0, 0.0)),   # scaled scene, photo-only upstream: wrapped 66 cells of the speculative tail before the guard
    (2, 0.04, 2.0, 0.5, (1.0, 0.5)),   # geometry gate closed -> fallback passes: wrapped 8 cells of the geometry pass
    (3, 0.04, 2.0, 0.0, None),         # no speculation: fallback passes (30 wraps before the guard)
])
def test_compressive_warps_do_not_wrap_the_fixed_point_window_fp32(lib, B, scale, tz, w_geom, hint):
    """Round-4 review: the fixed-point scatter cells (+-2048 units) wrap SILENTLY if more than 32 near-cap pixels of one
    tile pile on one reference texel.  Reachable (second half of the cases; errors of 70 .. 145 % of the map's scale were
    measured before round 5).  Round 5 let tiles with a small scatter footprint bypass the window (a heuristic); round 6
    derives the unit of a tile's cells from an upper bound of everything the tile can add to one of them
    (scsfm_geom.h: win_units_of), so that no cell can wrap whatever the warp does, and the fallback pass stages in floating
    cells.  Debug launches (SCSFM_DEBUG_CHECK_WINDOW) count wraps exactly: the count must be zero and dL/d ref_depth must
    match the fp64 oracle."""
    ti, K, ris, tds, rds, ps, pis = _compressive_case(B, scale, tz)
    c = lambda x: x.double()
    td64, rd64 = [leaf(c(tds[0]))], [[leaf(c(rds[0][0]))]]
    po, go = O.photo_and_geometry_loss(c(ti), [c(ris[0])], c(K), td64, rd64, [c(ps[0])], [c(pis[0])], 1, 1, 1, 1, "zeros")
    (po + w_geom * go).backward()
    fl = capi.make_flags(1, 1, 1, "zeros")
    photo, geom, outs, ws = capi.photo_geometry_fwd(lib, fl, ti, K, ris, tds, rds, ps, pis, hint=hint, check_window=hint is not None)
    assert abs(float(photo) - float(po)) < 1e-5 and abs(float(geom) - float(go)) < 1e-5
    g_td, g_rd, _, _ = capi.photo_geometry_bwd(lib, fl, ti, K, ris, tds, rds, ps, pis, ws, torch.tensor([1.0]),
                                               torch.tensor([w_geom]), check_window=True)  # (raises WindowOverflow on a wrap)
    assert capi.window_overflows(lib, ws, 2, B, 72, 100, spec=hint is not None) == [0, 0]
    assert _rel(g_rd[0][0].double(), rd64[0][0].grad) < 1e-4 and _rel(g_td[0].double(), td64[0].grad) < 1e-4


from _util import nonuniform_case as _nonuniform_case  # noqa: E402  (shared with the hardware twin in tests/test_gpu_parity.py)


@pytest.mark.parametrize("auto", [0, 1])
def test_nonuniform_compression_inside_a_large_footprint_fp32(lib, auto):
    ti, K, ris, tds, rds, ps, pis = _nonuniform_case()
    c = lambda x: x.double()
    td64, rd64 = [leaf(c(tds[0]))], [[leaf(c(rds[0][0]))]]
    po, go = O.photo_and_geometry_loss(c(ti), [c(ris[0])], c(K), td64, rd64, [c(ps[0])], [c(pis[0])], 1, 1, 1, auto, "zeros")
    po.backward()
    fl = capi.make_flags(1, 1, auto, "zeros")
    photo, geom, outs, ws = capi.photo_geometry_fwd(lib, fl, ti, K, ris, tds, rds, ps, pis, hint=(1.0, 0.0), check_window=True)
    assert abs(float(photo) - float(po)) < 1e-5 and abs(float(geom) - float(go)) < 1e-5
    g_td, g_rd, _, _ = capi.photo_geometry_bwd(lib, fl, ti, K, ris, tds, rds, ps, pis, ws, torch.tensor([1.0]),
                                               torch.tensor([0.0]), check_window=True)
    assert capi.window_overflows(lib, ws, 2, 2, 72, 100) == [0, 0]
    # the case is what it claims to be: the terms piled on the busiest reference texel exceed a 2^-20 cell's range
    unscaled = rd64[0][0].grad.abs().max() * 3 * float(outs[0, 4])
    assert float(unscaled) > 2048, float(unscaled)
    assert _rel(g_rd[0][0].double(), rd64[0][0].grad) < 1e-4 and _rel(g_td[0].double(), td64[0].grad) < 1e-4


def test_the_wrap_detector_fires_without_the_guard():
    """The same scaled scene on a build WITHOUT the per-tile bound of the cells' unit (-DSCSFM_WINDOW_BOUND=0, its own
    simulation library: every tile counts in 2^-20 as before round 6): cells wrap, dL/d ref_depth is off by multiples of
    4096 units, and the debug launch says so --
    capi.photo_geometry_fwd(check_window=True) raises WindowOverflow.  (A subprocess: the simulation's build flags are
    fixed at import.)"""
    import os
    import subprocess
    import sys
    code = """
import sys, torch
sys.path[:0] = [%r, %r, %r]
from hostsim import harness
from scsfm_hip import capi
import test_hostsim_kernels as T
lib = harness.lib()
ti, K, ris, tds, rds, ps, pis = T._compressive_case(3, 0.03, 2.0)
fl = capi.make_flags(1, 1, 1, "zeros")
_, _, outs, ws = capi.photo_geometry_fwd(lib, fl | capi.DEBUG_CHECK_WINDOW, ti, K, ris, tds, rds, ps, pis, hint=(1.0, 0.0))
n = capi.window_overflows(lib, ws, 2, 3, 72, 100)
assert n[0] > 0 and n[1] == 0 and float(outs[0, 7]) == n[0], (n, outs[:, 7])
try:
    capi.photo_geometry_fwd(lib, fl, ti, K, ris, tds, rds, ps, pis, hint=(1.0, 0.0), check_window=True)
except capi.WindowOverflow as e:
    print("RAISED", n[0])
""" % (os.path.dirname(os.path.abspath(__file__)), os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
       os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "sc-sfmlearner-release_amd"))
    env = dict(os.environ, HOSTSIM_EXTRA="-DSCSFM_WINDOW_BOUND=0")
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0 and "RAISED" in out.stdout, out.stdout[-1500:] + out.stderr[-3000:]


def test_coarse_maps_of_unsupported_shapes(lib, monkeypatch):
    """A coarser scale that is not an exact power-of-two reduction is up-sampled by F.interpolate in the shim (as the
    reference does) and still matches the oracle; maps of different scales within one pair are rejected by the
    library wrapper with check_sizes' message."""
    import loss_functions as LF
    from scsfm_hip import _lib, ops
    monkeypatch.setattr(_lib, "get", lambda: lib)
    monkeypatch.setattr(ops, "_need_cuda", lambda *a: None)
    B, H, W = 2, 72, 100
    d = synth.make_batch(B, H, W, n_ref=1, seed=58, depth="smooth", num_scales=2)
    c = lambda x: x.double().contiguous()
    ti, K, ris = c(d["tgt_img"]), c(d["intrinsics"]), [c(d["ref_imgs"][0])]
    odd = lambda t: c(F.interpolate(t, (H // 3, W // 3), mode="bilinear", align_corners=False))
    tds = [c(d["tgt_depth"][0]), odd(d["tgt_depth"][0])]
    rds = [[c(d["ref_depths"][0][0]), odd(d["ref_depths"][0][0])]]
    ps, pis = [c(d["poses"][0])], [c(d["poses_inv"][0])]
    td, rd = [leaf(t) for t in tds], [[leaf(t) for t in r] for r in rds]
    photo_o, geom_o = O.photo_and_geometry_loss(ti, ris, K, td, rd, ps, pis, 2, 1, 1, 1, "zeros")
    (photo_o + 0.5 * geom_o).backward()
    td2, rd2 = [leaf(t) for t in tds], [[leaf(t) for t in r] for r in rds]
    photo, geom = LF.compute_photo_and_geometry_loss(ti, ris, K, td2, rd2, ps, pis, 2, 1, 1, 1, "zeros")
    (photo + 0.5 * geom).backward()
    assert abs(float(photo) - float(photo_o)) < 1e-11 and abs(float(geom) - float(geom_o)) < 1e-11
    assert _rel(td2[1].grad, td[1].grad) < 1e-10 and _rel(rd2[0][1].grad, rd[0][1].grad) < 1e-10
    assert capi.depth_shift((B, 1, H // 2, W // 2), B, H, W) == 1 and capi.depth_shift((B, 1, H // 4, W // 4), B, H, W) == 2
    assert capi.depth_shift((B, 1, H // 8, W // 8), B, H, W) is None  # 100 is not a multiple of 8
    fl = capi.make_flags(1, 1, 1, "zeros")
    with pytest.raises(AssertionError, match="wrong size for depth"):
        capi.photo_geometry_fwd(lib, fl, ti, K, ris, [c(d["tgt_depth"][1])], [[c(d["ref_depths"][0][0])]], ps, pis)
    with pytest.raises(AssertionError, match="wrong size for depth"):  # scale 0 is never re-sampled
        LF.compute_photo_and_geometry_loss(ti, ris, K, [tds[1]], [[rds[0][1]]], ps, pis, 1, 1, 1, 1, "zeros")


@pytest.mark.parametrize("hint,upstream", [((1.0, 0.5), (1.0, 0.5)), ((1.0, 0.5), (0.3, 1.1)), (None, (1.0, 0.5))])
def test_no_result_depends_on_uninitialised_memory(lib, monkeypatch, hint, upstream):
    """Workspaces, scratch planes, loss rows and gradient buffers come from torch.empty.  With every such
    allocation poisoned (all-ones bytes = NaN) the step must give exactly what it gives on clean memory:
    everything that is read was written first, and the batched backwards store rather than accumulate."""
    d = synth.make_batch(2, 72, 100, n_ref=2, seed=31, depth="smooth")
    c = lambda x: x.double().contiguous()
    ti, K = c(d["tgt_img"]), c(d["intrinsics"])
    ris = [c(r) for r in d["ref_imgs"]]
    tds, rds = [c(d["tgt_depth"][0])], [[c(r[0])] for r in d["ref_depths"]]
    ps, pis = [c(p) for p in d["poses"]], [c(p) for p in d["poses_inv"]]
    fl = capi.make_flags(1, 1, 1, "zeros")
    gp = torch.tensor([upstream[0]], dtype=torch.float64)
    gg = torch.tensor([upstream[1]], dtype=torch.float64)

    def step():
        photo, geom, _, ws = capi.photo_geometry_fwd(lib, fl, ti, K, ris, tds, rds, ps, pis, hint=hint)
        g = capi.photo_geometry_bwd(lib, fl, ti, K, ris, tds, rds, ps, pis, ws, gp, gg)
        sm, sws = capi.smooth_multi_fwd(lib, tds + [r[0] for r in rds], [ti] + ris)
        gs = capi.smooth_multi_bwd(lib, tds + [r[0] for r in rds], [ti] + ris, sws, torch.ones(1, dtype=torch.float64))
        flat = [g[0][0]] + [r[0] for r in g[1]] + list(g[2]) + list(g[3]) + list(gs)
        return [photo.clone(), geom.clone(), sm.clone()] + [t.clone() for t in flat]

    clean = step()
    real_empty = torch.empty

    def poisoned(*a, **k):
        t = real_empty(*a, **k)
        if t.dtype == torch.uint8:
            t.fill_(255)
        elif t.is_floating_point():
            t.fill_(float("nan"))
        return t

    monkeypatch.setattr(torch, "empty", poisoned)
    dirty = step()
    monkeypatch.undo()
    for a, b in zip(dirty, clean):
        assert torch.equal(a, b)


@pytest.mark.parametrize("hint,upstream", [((0.7, 1.3), (0.7, 1.3)), ((0.7, 1.3), (1.0, 0.5)), (None, (0.7, 1.3))])
def test_thread_and_block_order_do_not_matter(lib, monkeypatch, hint, upstream):
    """HOSTSIM_ORDER=reverse runs the threads of every workgroup, and the workgroups of every grid, in
    descending order.  The fused kernels (LDS tiles re-used for parking, window, reduction scratch) must still
    reproduce the oracle: a dependence on the order in which threads run between two barriers is a data race."""
    monkeypatch.setenv("HOSTSIM_ORDER", "reverse")
    test_speculative_forward_fp64(lib, hint, upstream)
    test_smooth_matches_oracle_and_golden(lib)


@pytest.mark.parametrize("H,W,B", [(15, 63, 40), (33, 129, 8), (5, 200, 40)])
@pytest.mark.parametrize("hint", [(1.0, 0.5), None])
def test_odd_image_sizes_with_open_gates(lib, H, W, B, hint):
    """Sizes that are no multiple of any tile (a last partial tile in both directions, images narrower than a
    wave or lower than a strip), with enough pixels in the batch that the 10000-pixel gates are open, against
    the fp64 oracle: the fused forward + combine, and the plain forward + the backward's two passes."""
    d = synth.make_batch(B, H, W, n_ref=1, seed=H * 100 + W, depth="smooth")
    c = lambda x: x.double().contiguous()
    ti, K = c(d["tgt_img"]), c(d["intrinsics"])
    ris = [c(r) for r in d["ref_imgs"]]
    tds, rds = [c(d["tgt_depth"][0])], [[c(r[0])] for r in d["ref_depths"]]
    ps, pis = [c(p) for p in d["poses"]], [c(p) for p in d["poses_inv"]]
    td, rd = [leaf(t) for t in tds], [[leaf(t) for t in r] for r in rds]
    pp, pi = [leaf(p) for p in ps], [leaf(p) for p in pis]
    po, go = O.photo_and_geometry_loss(ti, ris, K, td, rd, pp, pi, 1, 1, 1, 1, "zeros")
    assert float(po) > 0 and float(go) > 0  # gates open
    (1.0 * po + 0.5 * go).backward()
    fl = capi.make_flags(1, 1, 1, "zeros")
    photo, geom, _, ws = capi.photo_geometry_fwd(lib, fl, ti, K, ris, tds, rds, ps, pis, hint=hint)
    assert abs(float(photo) - float(po)) < 1e-12 and abs(float(geom) - float(go)) < 1e-12
    one, half = torch.tensor([1.0], dtype=torch.float64), torch.tensor([0.5], dtype=torch.float64)
    g_td, g_rd, g_p, g_pi = capi.photo_geometry_bwd(lib, fl, ti, K, ris, tds, rds, ps, pis, ws, one, half)
    assert _rel(g_td[0], td[0].grad) < 1e-10 and _rel(g_rd[0][0], rd[0][0].grad) < 1e-10
    assert _rel(g_p[0], pp[0].grad) < 1e-10 and _rel(g_pi[0], pi[0].grad) < 1e-10


@pytest.mark.parametrize("n_scales", [1, 2])
def test_single_node_step_equals_the_three_reference_style_calls(lib, monkeypatch, n_scales):
    """compute_total_loss (one autograd node: both losses + the weighted sum) against
    compute_photo_and_geometry_loss + compute_smooth_loss + w1*l1 + w2*l2 + w3*l3, values and gradients, fp64,
    through the autograd nodes with the host-simulation library."""
    import loss_functions as LF
    from scsfm_hip import _lib, ops
    monkeypatch.setattr(_lib, "get", lambda: lib)
    monkeypatch.setattr(ops, "_need_cuda", lambda *a: None)
    H, W = 72, 100
    d = synth.make_batch(2, H, W, n_ref=2, seed=41, depth="smooth", num_scales=n_scales)
    c = lambda x: x.double().contiguous()
    ti, K = c(d["tgt_img"]), c(d["intrinsics"])
    ris = [c(r) for r in d["ref_imgs"]]
    w1, w2, w3 = 1.0, 0.1, 0.5

    def leaves():
        return ([leaf(c(t)) for t in d["tgt_depth"]], [[leaf(c(t)) for t in r] for r in d["ref_depths"]],
                [leaf(c(p)) for p in d["poses"]], [leaf(c(p)) for p in d["poses_inv"]])

    td, rd, pp, pi = leaves()
    photo, geom = LF.compute_photo_and_geometry_loss(ti, ris, K, td, rd, pp, pi, n_scales, 1, 1, 1, "zeros")
    smooth = LF.compute_smooth_loss(td, ti, rd, ris)
    (w1 * photo + w2 * smooth + w3 * geom).backward()
    td2, rd2, pp2, pi2 = leaves()
    loss, l1, l2, l3 = LF.compute_total_loss(ti, ris, K, td2, rd2, pp2, pi2, n_scales, 1, 1, 1, "zeros", w1, w2, w3)
    assert not l1.requires_grad and not l2.requires_grad and not l3.requires_grad
    loss.backward()
    assert abs(float(l1) - float(photo)) < 1e-14 and abs(float(l2) - float(smooth)) < 1e-14
    assert abs(float(l3) - float(geom)) < 1e-14
    assert abs(float(loss) - float(w1 * photo + w2 * smooth + w3 * geom)) < 1e-13
    for a, b in zip(td + [t for r in rd for t in r] + pp + pi, td2 + [t for r in rd2 for t in r] + pp2 + pi2):
        assert _rel(b.grad, a.grad) < 1e-11


def test_single_node_step_with_more_frames_than_one_fused_launch(lib, monkeypatch):
    """Target + 8 references = 9 frames > the 8 one launch of scsfm_smooth_multi_fwd_step holds (and 16 pair-directions
    = two launches per pair stage): compute_total_loss falls back to the reference's call structure instead of raising
    (round-4 advisor finding); values and gradients against the oracle, fp64."""
    import loss_functions as LF
    from scsfm_hip import _lib, ops
    monkeypatch.setattr(_lib, "get", lambda: lib)
    monkeypatch.setattr(ops, "_need_cuda", lambda *a: None)
    n_ref = 8
    assert 1 + n_ref > LF.MAX_FUSED_FRAMES
    d = synth.make_batch(4, 48, 80, n_ref=n_ref, seed=43, depth="smooth")  # (enough pixels to open the 10000-pixel gates)
    c = lambda x: x.double().contiguous()
    ti, K, ris = c(d["tgt_img"]), c(d["intrinsics"]), [c(r) for r in d["ref_imgs"]]
    w1, w2, w3 = 1.0, 0.1, 0.5

    def leaves():
        return ([leaf(c(t)) for t in d["tgt_depth"]], [[leaf(c(t)) for t in r] for r in d["ref_depths"]],
                [leaf(c(p)) for p in d["poses"]], [leaf(c(p)) for p in d["poses_inv"]])

    td, rd, pp, pi = leaves()
    photo, geom = O.photo_and_geometry_loss(ti, ris, K, td, rd, pp, pi, 1, 1, 1, 1, "zeros")
    smooth = O.smooth_loss(td, ti, rd, ris)
    (w1 * photo + w2 * smooth + w3 * geom).backward()
    td2, rd2, pp2, pi2 = leaves()
    loss, l1, l2, l3 = LF.compute_total_loss(ti, ris, K, td2, rd2, pp2, pi2, 1, 1, 1, 1, "zeros", w1, w2, w3)
    assert not l1.requires_grad and not l2.requires_grad and not l3.requires_grad
    loss.backward()
    assert abs(float(l1) - float(photo)) < 1e-11 and abs(float(l2) - float(smooth)) < 1e-11 and abs(float(l3) - float(geom)) < 1e-11
    assert float(photo) > 0 and float(geom) > 0
    for a, b in zip(td + [t for r in rd for t in r] + pp + pi, td2 + [t for r in rd2 for t in r] + pp2 + pi2):
        assert _rel(b.grad, a.grad) < 1e-10


@pytest.mark.parametrize("H,W,dtype,hint,upstream", [
    (72, 100, torch.float64, (1.0, 0.5), (1.0, 0.5)),    # speculation holds: guards + combine
    (15, 63, torch.float64, (1.0, 0.5), (0.3, 1.1)),     # odd plane (945 elements: no 16-byte path), fallback passes
    (33, 129, torch.float32, (1.0, 0.5), (1.0, 0.5)),    # fp32, plane not a multiple of 4
    (40, 92, torch.float32, None, (0.7, 1.3)),           # fp32, 16-byte path, plain forward
])
def test_smooth_gradient_rides_along_in_the_combining_pass(lib, H, W, dtype, hint, upstream):
    """scsfm_pairs_bwd_smooth (ABI 8): the smooth term's depth gradients added by the pass that stores the pair terms'
    must equal scsfm_pairs_bwd followed by scsfm_smooth_multi_bwd(accumulate) -- the same additions in another order, so
    to round-off -- for every frame, on the 16-byte and the scalar paths, after a speculative and after a plain forward."""
    B = 3
    d = synth.make_batch(B, H, W, n_ref=2, seed=7, depth="smooth")
    c = lambda x: x.to(dtype).contiguous()
    ti, K, ris = c(d["tgt_img"]), c(d["intrinsics"]), [c(r) for r in d["ref_imgs"]]
    tds, rds = [c(d["tgt_depth"][0])], [[c(r[0])] for r in d["ref_depths"]]
    ps, pis = [c(p) for p in d["poses"]], [c(p) for p in d["poses_inv"]]
    fl = capi.make_flags(1, 1, 1, "zeros")
    t = lambda v: torch.tensor([v], dtype=dtype)
    frames, imgs = [tds[0]] + [r[0] for r in rds], [ti] + ris
    _, sws = capi.smooth_multi_fwd(lib, frames, imgs, keep_edges=True)
    gs = t(0.37)

    def run(fused):
        _, _, _, ws = capi.photo_geometry_fwd(lib, fl, ti, K, ris, tds, rds, ps, pis, hint=hint)
        res = capi.photo_geometry_bwd(lib, fl, ti, K, ris, tds, rds, ps, pis, ws, t(upstream[0]), t(upstream[1]),
                                      smooth=(sws, gs) if fused else None)
        g_td, g_rd, g_p, g_pi = res[:4]
        if not fused:
            capi.smooth_multi_bwd(lib, frames, imgs, sws, gs, into=[g_td[0]] + [r[0] for r in g_rd])
        return [g_td[0].clone()] + [r[0].clone() for r in g_rd] + [x.clone() for x in g_p + g_pi]

    a, b = run(True), run(False)
    tol = 1e-12 if dtype == torch.float64 else 2e-6
    for k, (x, y) in enumerate(zip(a, b)):
        assert k >= 3 or float(y.abs().max()) > 0   # (the small case is below the 10000-pixel gate: its pair terms are 0)
        assert float((x - y).abs().max()) <= tol * max(float(y.abs().max()), 1e-30)
    # ... and the smooth part alone is what it should be: fused minus a pair-only backward
    _, _, _, ws = capi.photo_geometry_fwd(lib, fl, ti, K, ris, tds, rds, ps, pis, hint=hint)
    res = capi.photo_geometry_bwd(lib, fl, ti, K, ris, tds, rds, ps, pis, ws, t(upstream[0]), t(upstream[1]))
    only = capi.smooth_multi_bwd(lib, frames, imgs, sws, gs)
    for x, y, z in zip(a[:3], [res[0][0]] + [r[0] for r in res[1]], only):
        assert _rel(x - y, z) < (1e-9 if dtype == torch.float64 else 2e-3)


from _spec_rule import sums_of as _sums_of  # noqa: E402  (double[16] of pair j's workspace; shared with the hardware tests)


def test_the_device_side_hint_follows_the_upstream_gradients(lib):
    """scsfm_pair_desc::hint: a training loop with other loss weights than the host hint (here -p 1 -c 0.3 against the
    default 1 : 0.5) mis-speculates ONCE.  The backward falls back to its own passes, leaves the weights it saw on the
    device, and from the next step on the forward speculates on them: its results stand (the workspace still carries a
    valid speculation after the backward) and the gradients equal the oracle's either way."""
    B, H, W = 4, 72, 100
    d = synth.make_batch(B, H, W, n_ref=1, seed=41, depth="smooth")
    c = lambda x: x.double().contiguous()
    ti, K = c(d["tgt_img"]), c(d["intrinsics"])
    ris = [c(r) for r in d["ref_imgs"]]
    tds, rds = [c(d["tgt_depth"][0])], [[c(r[0])] for r in d["ref_depths"]]
    ps, pis = [c(p) for p in d["poses"]], [c(p) for p in d["poses_inv"]]
    fl = capi.make_flags(1, 1, 1, "zeros")
    up = (1.0, 0.3)
    td, rd = [leaf(t) for t in tds], [[leaf(t) for t in r] for r in rds]
    pp, pi = [leaf(p) for p in ps], [leaf(p) for p in pis]
    po, go = O.photo_and_geometry_loss(ti, ris, K, td, rd, pp, pi, 1, 1, 1, 1, "zeros")
    assert float(go) > 0  # the geometry gate is open: the ratio matters
    (up[0] * po + up[1] * go).backward()
    hint_dev = torch.tensor([1.0, 0.5], dtype=torch.float64)
    t = lambda v: torch.tensor([v], dtype=torch.float64)
    held = []
    for step in range(3):
        photo, geom, _, ws = capi.photo_geometry_fwd(lib, fl, ti, K, ris, tds, rds, ps, pis, hint=(1.0, 0.5), hint_dev=hint_dev)
        assert abs(float(photo) - float(po)) < 1e-12 and abs(float(geom) - float(go)) < 1e-12
        g_td, g_rd, g_p, g_pi = capi.photo_geometry_bwd(lib, fl, ti, K, ris, tds, rds, ps, pis, ws, t(up[0]), t(up[1]),
                                                        hint_dev=hint_dev)
        assert _rel(g_td[0], td[0].grad) < 1e-10 and _rel(g_rd[0][0], rd[0][0].grad) < 1e-10, step
        assert _rel(g_p[0], pp[0].grad) < 1e-10 and _rel(g_pi[0], pi[0].grad) < 1e-10, step
        assert hint_dev.tolist() == [1.0, 0.3]
        # sums[8]: still a valid speculation after the backward (1) or retired by the fallback (0)
        held.append([float(_sums_of(lib, ws, j, B, H, W)[8]) for j in range(2)])
    assert held == [[0.0, 0.0], [1.0, 1.0], [1.0, 1.0]], held
    # a backward whose upstream gradients are not finite (the overflow step of a loss-scaled run) leaves the hint alone
    for bad in (float("nan"), float("inf")):
        photo, geom, _, ws = capi.photo_geometry_fwd(lib, fl, ti, K, ris, tds, rds, ps, pis, hint=(1.0, 0.5), hint_dev=hint_dev)
        capi.photo_geometry_bwd(lib, fl, ti, K, ris, tds, rds, ps, pis, ws, t(bad), t(0.3), hint_dev=hint_dev)
        assert hint_dev.tolist() == [1.0, 0.3]
    # a backward with a zero photometric weight: nothing to factor out next time, the forward says so itself
    photo, geom, _, ws = capi.photo_geometry_fwd(lib, fl, ti, K, ris, tds, rds, ps, pis, hint=(1.0, 0.5), hint_dev=hint_dev)
    capi.photo_geometry_bwd(lib, fl, ti, K, ris, tds, rds, ps, pis, ws, t(0.0), t(0.7), hint_dev=hint_dev)
    assert hint_dev.tolist() == [0.0, 0.7]
    photo, geom, _, ws = capi.photo_geometry_fwd(lib, fl, ti, K, ris, tds, rds, ps, pis, hint=(1.0, 0.5), hint_dev=hint_dev)
    assert float(_sums_of(lib, ws, 0, B, H, W)[8]) == 0.0
    td2, rd2 = [leaf(x) for x in tds], [[leaf(x) for x in r] for r in rds]
    pp2, pi2 = [leaf(p) for p in ps], [leaf(p) for p in pis]
    po2, go2 = O.photo_and_geometry_loss(ti, ris, K, td2, rd2, pp2, pi2, 1, 1, 1, 1, "zeros")
    (0.0 * po2 + 0.7 * go2).backward()
    g_td, g_rd, g_p, g_pi = capi.photo_geometry_bwd(lib, fl, ti, K, ris, tds, rds, ps, pis, ws, t(0.0), t(0.7), hint_dev=hint_dev)
    assert _rel(g_td[0], td2[0].grad) < 1e-10 and _rel(g_p[0], pp2[0].grad) < 1e-10
