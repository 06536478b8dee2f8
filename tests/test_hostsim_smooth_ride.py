"""The smooth loss riding in the speculative forward (round 6; scsfm_pair_desc::smooth_ws, loss_functions.py:132-159 next to
:50-92 as train.py:262-268 calls them) in the CPU simulation of the product sources: against the stand-alone smooth forward
(the edge planes and the per-image records it leaves must be THE SAME -- the backward entry points are shared), against the
fp64 oracle, and with the pair losses of the same call untouched."""
import numpy as np
import pytest
import torch

from hostsim import harness
from oracle import scsfm_oracle as O
from scsfm_hip import capi, synth

CASES = [  # B, H, W, n_ref, dtype, depth law
    (4, 72, 100, 2, torch.float32, "smooth"),
    (3, 41, 150, 2, torch.float32, "scene"),   # partial tiles in both directions
    (2, 30, 63, 1, torch.float32, "iid"),      # one reference: two pair-directions, two frames
    (2, 33, 70, 3, torch.float64, "smooth"),   # fp64 instantiation (8-row tiles), three references
]


@pytest.fixture(scope="module")
def lib():
    return harness.lib()


def _inputs(B, H, W, n_ref, dtype, depth):
    d = synth.make_batch(B, H, W, n_ref=n_ref, seed=11 + H, depth=depth)
    c = lambda t: t.to(dtype).contiguous()
    return (c(d["tgt_img"]), c(d["intrinsics"]), [c(r) for r in d["ref_imgs"]], [c(d["tgt_depth"][0])],
            [[c(r[0])] for r in d["ref_depths"]], [c(p) for p in d["poses"]], [c(p) for p in d["poses_inv"]])


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(map(str, c)))
def test_smooth_loss_riding_in_the_speculative_forward(lib, case):
    B, H, W, n_ref, dtype, depth = case
    ti, K, ris, tds, rds, ps, pis = _inputs(B, H, W, n_ref, dtype, depth)
    fl = capi.make_flags(1, 1, 1, "zeros")
    hint = (1.0, 0.5)
    assert capi.smooth_rides_along(fl, ti, tds, rds, hint)
    photo0, geom0, outs0, _ = capi.photo_geometry_fwd(lib, fl, ti, K, ris, tds, rds, ps, pis, hint=hint)
    photo, geom, outs, ws, smooth, sws = capi.photo_geometry_fwd(lib, fl, ti, K, ris, tds, rds, ps, pis, hint=hint, smooth=True)
    # the pair losses do not notice the passenger
    assert torch.equal(outs0, outs) and float(photo0) == float(photo) and float(geom0) == float(geom)
    frames, imgs = tds + [r[0] for r in rds], [ti] + ris
    ref_loss, ref_ws = capi.smooth_multi_fwd(lib, frames, imgs, keep_edges=True)
    nf = len(frames)
    sw_bytes = capi._sizes(lib, B, H, W)[2]
    plane_bytes = ((B * H * W * ti.element_size() + 255) // 256) * 256
    assert sws.numel() == ref_ws.numel() == nf * (sw_bytes + plane_bytes)
    for f in range(nf):
        e = lambda w: w[nf * sw_bytes + f * plane_bytes:nf * sw_bytes + f * plane_bytes + B * H * W * ti.element_size()].view(dtype)
        assert torch.equal(e(sws), e(ref_ws)), f"edge plane of frame {f}"
        s = lambda w: w[f * sw_bytes:f * sw_bytes + 16 * B].view(torch.float64)
        # {mean + 1e-7, L} per image: the same sums in another grouping
        assert torch.allclose(s(sws), s(ref_ws), rtol=1e-6 if dtype == torch.float32 else 1e-13, atol=0)
    tol = 1e-6 if dtype == torch.float32 else 1e-12
    assert abs(float(smooth) - float(ref_loss)) <= tol * max(1.0, abs(float(ref_loss)))
    c = lambda x: x.double()
    want = O.smooth_loss([c(t) for t in tds], c(ti), [[c(r[0])] for r in rds], [c(r) for r in ris])
    assert abs(float(smooth) - float(want)) <= (1e-5 if dtype == torch.float32 else 1e-10)
    # the shared backward takes the workspace from there
    g = torch.ones(1, dtype=dtype)
    ga = capi.smooth_multi_bwd(lib, frames, imgs, sws, g)
    gb = capi.smooth_multi_bwd(lib, frames, imgs, ref_ws, g)
    for a, b in zip(ga, gb):
        assert float((a - b).abs().max()) <= (1e-6 if dtype == torch.float32 else 1e-13) * float(b.abs().max())  # (den in another grouping)


def test_step_total_formed_by_the_finalize_launch(lib):
    B, H, W = 4, 72, 100
    ti, K, ris, tds, rds, ps, pis = _inputs(B, H, W, 2, torch.float32, "smooth")
    fl = capi.make_flags(1, 1, 1, "zeros")
    w = (1.0, 0.1, 0.5)
    photo, geom, _, _, smooth, _, out = capi.photo_geometry_fwd(lib, fl, ti, K, ris, tds, rds, ps, pis, hint=(w[0], w[2]),
                                                                smooth=True, step=w)
    want = torch.tensor([w[0] * float(photo) + w[1] * float(smooth) + w[2] * float(geom), float(photo), float(smooth), float(geom)])
    assert torch.allclose(out, want, rtol=1e-6, atol=0)


def test_descriptors_the_fold_cannot_serve_are_rejected(lib):
    """smooth_ws on a plain (non-speculative) forward or on a coarser scale is an argument error, not a silent skip."""
    import ctypes as ct
    B, H, W = 2, 32, 64
    ti, K, ris, tds, rds, ps, pis = _inputs(B, H, W, 1, torch.float32, "smooth")
    ws_bytes, scratch_bytes, sw_bytes = capi._sizes(lib, B, H, W)
    ws = torch.empty(ws_bytes + scratch_bytes, dtype=torch.uint8)
    sws = torch.empty(sw_bytes, dtype=torch.uint8)
    out = torch.empty(8)
    d = (capi.PairDesc * 1)()
    d[0].tgt_img, d[0].ref_img, d[0].tgt_depth, d[0].ref_depth, d[0].pose = ti.data_ptr(), ris[0].data_ptr(), \
        tds[0].data_ptr(), rds[0][0].data_ptr(), ps[0].data_ptr()
    d[0].ws, d[0].out, d[0].smooth_ws = ws.data_ptr(), out.data_ptr(), sws.data_ptr()
    call = lambda wp: lib._fn["scsfm_pairs_fwd_f32"](1, ct.addressof(d), B, H, W, K.data_ptr(), 7, wp, 0.5, 0)
    assert call(1.0) == -1            # no gbuf: the plain forward
    d[0].gbuf = ws.data_ptr() + ws_bytes
    assert call(0.0) == -1            # a gbuf, but nothing to speculate on
    assert call(1.0) == 0             # the speculative forward carries it


def test_smooth_total_without_total_is_rejected(lib):
    """scsfm_pair_desc::smooth_total is formed by the workgroup that finishes d[0].total: set without it, the value was
    never written and the call returned 0.  Now SCSFM_ERR_ARG from all four entry points, and nothing is launched: the
    output buffers keep their bits."""
    import ctypes as ct
    B, H, W = 2, 32, 64
    for dtype, sfx in ((torch.float32, "f32"), (torch.float64, "f64")):
        ti, K, ris, tds, rds, ps, pis = _inputs(B, H, W, 1, dtype, "smooth")
        ws_bytes, scratch_bytes, sw_bytes = capi._sizes(lib, B, H, W)
        ws = torch.full((ws_bytes + scratch_bytes,), 0xA5, dtype=torch.uint8)
        sws = torch.full((sw_bytes,), 0xA5, dtype=torch.uint8)
        out, souts, step_out = (torch.full((n,), -77.25, dtype=dtype) for n in (10, 2, 4))
        d = (capi.PairDesc * 1)()
        d[0].tgt_img, d[0].ref_img, d[0].tgt_depth, d[0].ref_depth, d[0].pose = ti.data_ptr(), ris[0].data_ptr(), \
            tds[0].data_ptr(), rds[0][0].data_ptr(), ps[0].data_ptr()
        d[0].ws, d[0].gbuf, d[0].out, d[0].smooth_ws = ws.data_ptr(), ws.data_ptr() + ws_bytes, out.data_ptr(), sws.data_ptr()
        d[0].smooth_out, d[0].smooth_total = souts.data_ptr(), souts.data_ptr() + souts.element_size()
        fwd = lambda: lib._fn[f"scsfm_pairs_fwd_{sfx}"](1, ct.addressof(d), B, H, W, K.data_ptr(), 7, 1.0, 0.5, 0)
        step = lambda: lib._fn[f"scsfm_pairs_fwd_step_{sfx}"](1, ct.addressof(d), B, H, W, K.data_ptr(), 7, 1.0, 0.1, 0.5,
                                                              step_out.data_ptr(), 0)
        assert d[0].total is None
        assert fwd() == -1 and step() == -1
        untouched = lambda: bool((ws == 0xA5).all()) and bool((sws == 0xA5).all()) and \
            all(bool((t == -77.25).all()) for t in (out, souts, step_out))
        assert untouched()
        d[0].smooth_total = None  # without either total the plain call is served ...
        assert fwd() == 0 and float(souts[1]) == -77.25 and float(souts[0]) != -77.25
        d[0].smooth_total, d[0].total = souts.data_ptr() + souts.element_size(), out.data_ptr() + 8 * out.element_size()
        assert fwd() == 0 and step() == 0  # ... and with both
        assert float(souts[1]) == float(souts[0]) and float(step_out[2]) == float(souts[0])
        assert abs(float(step_out[0]) - (float(out[8]) + 0.1 * float(souts[0]) + 0.5 * float(out[9]))) <= 1e-6


# ---- the host mirror: the reference's two calls (train.py:262-266) with the smooth loss found waiting -----------------
@pytest.fixture()
def on_sim(lib, monkeypatch):
    from scsfm_hip import _lib, config, ops
    monkeypatch.setattr(_lib, "get", lambda: lib)
    monkeypatch.setattr(ops, "_need_cuda", lambda *a: None)
    calls = {"smooth_fwd": 0}
    real = capi.smooth_multi_fwd

    def counted(*a, **k):
        calls["smooth_fwd"] += 1
        return real(*a, **k)

    monkeypatch.setattr(capi, "smooth_multi_fwd", counted)
    prev = config.smooth_rides_along()
    yield calls
    config.set_smooth_rides_along(prev)
    ops._SmoothStash.slot = None


def _leaves(B=3, H=50, W=90, n_ref=2, seed=5):
    d = synth.make_batch(B, H, W, n_ref=n_ref, seed=seed, depth="smooth")
    lf = lambda t: t.clone().requires_grad_(True)
    return (d["tgt_img"], d["ref_imgs"], d["intrinsics"], [lf(d["tgt_depth"][0])], [[lf(r[0])] for r in d["ref_depths"]],
            [lf(p) for p in d["poses"]], [lf(p) for p in d["poses_inv"]])


def _reference_calls(x, between=None):
    import loss_functions as LF
    ti, ris, K, td, rd, ps, pis = x
    photo, geom = LF.compute_photo_and_geometry_loss(ti, ris, K, td, rd, ps, pis, 1, 1, 1, 1, "zeros")
    if between is not None:
        between(x)
    smooth = LF.compute_smooth_loss(td, ti, rd, ris)
    (1.0 * photo + 0.1 * smooth + 0.5 * geom).backward()
    grads = [td[0].grad] + [r[0].grad for r in rd] + [p.grad for p in ps + pis]
    return float(photo.detach()), float(smooth.detach()), float(geom.detach()), [g.clone() for g in grads]


def test_compute_smooth_loss_finds_its_result_waiting(on_sim):
    from scsfm_hip import config
    config.set_smooth_rides_along(False)
    want = _reference_calls(_leaves())
    assert on_sim["smooth_fwd"] == 1
    config.set_smooth_rides_along(True)
    got = _reference_calls(_leaves())
    assert on_sim["smooth_fwd"] == 1, "the stand-alone smooth forward ran although the speculative forward carried it"
    assert got[0] == want[0] and got[2] == want[2] and abs(got[1] - want[1]) <= 1e-6 * abs(want[1])
    for a, b in zip(got[3], want[3]):
        assert float((a - b).abs().max()) <= 1e-6 * float(b.abs().max())


def test_a_stale_or_foreign_stash_is_not_used(on_sim):
    """An in-place write into a depth map between the two calls, or other tensor objects (even with equal values), miss."""
    from scsfm_hip import config
    config.set_smooth_rides_along(True)

    import loss_functions as LF
    ti, ris, K, td, rd, ps, pis = _leaves()
    LF.compute_photo_and_geometry_loss(ti, ris, K, td, rd, ps, pis, 1, 1, 1, 1, "zeros")
    with torch.no_grad():
        td[0].mul_(1.5)  # the target depth map changes: what waits in the stash is the loss of the OLD map
    got = float(LF.compute_smooth_loss(td, ti, rd, ris))  # (forward only: autograd itself refuses a backward through the old map)
    assert on_sim["smooth_fwd"] == 1
    config.set_smooth_rides_along(False)
    want = float(LF.compute_smooth_loss(td, ti, rd, ris))
    assert abs(got - want) <= 1e-6 * abs(want)  # the smooth loss of the map as compute_smooth_loss saw it
    # other objects: the second call gets clones
    config.set_smooth_rides_along(True)
    ti, ris, K, td, rd, ps, pis = _leaves()
    n0 = on_sim["smooth_fwd"]
    LF.compute_photo_and_geometry_loss(ti, ris, K, td, rd, ps, pis, 1, 1, 1, 1, "zeros")
    LF.compute_smooth_loss([td[0].clone()], ti, [[r[0].clone()] for r in rd], ris)
    assert on_sim["smooth_fwd"] == n0 + 1
    # ... and a hit is consumed: a second compute_smooth_loss on the same frames computes
    LF.compute_photo_and_geometry_loss(ti, ris, K, td, rd, ps, pis, 1, 1, 1, 1, "zeros")
    a = LF.compute_smooth_loss(td, ti, rd, ris)
    b = LF.compute_smooth_loss(td, ti, rd, ris)
    assert on_sim["smooth_fwd"] == n0 + 2 and abs(float(a) - float(b)) <= 1e-6 * abs(float(b))


def test_single_node_step_with_the_smooth_loss_riding(on_sim):
    from scsfm_hip import config
    import loss_functions as LF

    def step(x):
        ti, ris, K, td, rd, ps, pis = x
        loss, photo, smooth, geom = LF.compute_total_loss(ti, ris, K, td, rd, ps, pis, 1, 1, 1, 1, "zeros", 1.0, 0.1, 0.5)
        loss.backward()
        return [float(v) for v in (loss, photo, smooth, geom)], [td[0].grad] + [r[0].grad for r in rd] + [p.grad for p in ps + pis]

    config.set_smooth_rides_along(False)
    v0, g0 = step(_leaves())
    n0 = on_sim["smooth_fwd"]
    config.set_smooth_rides_along(True)
    v1, g1 = step(_leaves())
    assert on_sim["smooth_fwd"] == n0  # no stand-alone smooth forward
    for a, b in zip(v1, v0):
        assert abs(a - b) <= 1e-6 * abs(b)
    for a, b in zip(g1, g0):
        assert float((a - b).abs().max()) <= 1e-6 * float(b.abs().max())


def test_each_loss_can_be_differentiated_on_its_own(on_sim):
    """The smooth loss found waiting is the third output of the pair losses' autograd node: its gradient normally arrives
    with theirs (one backward call, the smooth term added by the combining pass).  Differentiating only ONE of the three
    must still give that loss's gradients: the others' upstream gradients arrive as None and count as zero."""
    from scsfm_hip import config
    import loss_functions as LF

    def three(x, which):
        ti, ris, K, td, rd, ps, pis = x
        photo, geom = LF.compute_photo_and_geometry_loss(ti, ris, K, td, rd, ps, pis, 1, 1, 1, 1, "zeros")
        smooth = LF.compute_smooth_loss(td, ti, rd, ris)
        {"photo": photo, "geom": geom, "smooth": smooth, "all": photo + 0.1 * smooth + 0.5 * geom}[which].backward()
        z = lambda t: torch.zeros_like(t) if t.grad is None else t.grad.clone()
        return [z(td[0])] + [z(r[0]) for r in rd] + [z(p) for p in ps + pis]

    for which in ("smooth", "photo", "geom", "all"):
        config.set_smooth_rides_along(False)
        want = three(_leaves(), which)
        config.set_smooth_rides_along(True)
        n0 = on_sim["smooth_fwd"]
        got = three(_leaves(), which)
        assert on_sim["smooth_fwd"] == n0, which
        for a, b in zip(got, want):
            scale = float(b.abs().max())
            # (the two runs may take different routes to the same gradient: every backward leaves the upstream weights it saw
            # in the device-side hint, so the second run's forward speculates on them and its backward is the scaled add
            # of fixed-point planes where the first ran the fallback passes: 1e-6-sized differences)
            assert float((a - b).abs().max()) <= 2e-5 * scale + (0 if scale else 1e-30), which


# ---- the one-node step at other weights than 1 / 0.1 / 0.5: does its speculation stand, and are the gradients right? ---
import _spec_rule as R  # noqa: E402

STEP_WEIGHTS = [(1.0, 0.1, 0.5), (0.7, 0.1, 0.3), (1.0, 0.1, 0.3), (0.85, 0.05, 0.15), (1.0, 0.1, 0.1)]  # -p / -s / -c of a run
RULE_WEIGHTS = [(1.0, 0.1, 0.5), (1.0, 0.1, 0.3), (0.7, 0.1, 0.3)]
RULE_GRADIENTS = [1 / 3, 3.7, 1 / 12]


@pytest.fixture(scope="module")
def step_case():
    return {dt: R.inputs(dt) for dt in (torch.float32, torch.float64)}


@pytest.mark.parametrize("g_loss", [1.0, 0.125, 65536.0])
@pytest.mark.parametrize("w", STEP_WEIGHTS, ids=lambda w: "-".join(map(str, w)))
def test_speculation_stands_for_the_weights_a_run_can_have(lib, step_case, w, g_loss):
    """StepLoss's library calls in fp32 with upstream gradients that are powers of two (1, a loss scaler's scales): the
    forward stores the weights ROUNDED TO fp32, every pair-direction's speculation stands after the backward (sums[8] ==
    1), and the gradients equal the fp64 oracle's.  (With the unrounded doubles in sums[9..10] every triple but the
    first one ran the fallback passes on every step.)"""
    stored = (float(np.float32(w[0])), float(np.float32(w[2])))
    assert R.spec_holds(w[0], w[2], g_loss, torch.float32, stored)
    R.check_step(lib, step_case[torch.float32], w, g_loss, True, stored=stored)


def test_the_rule_table_has_both_outcomes():
    for dt, T in ((torch.float32, np.float32), (torch.float64, np.float64)):
        got = {R.spec_holds(w[0], w[2], g, dt, (float(T(w[0])), float(T(w[2])))) for w in RULE_WEIGHTS for g in RULE_GRADIENTS}
        assert got == {True, False}, dt
        assert all(R.spec_holds(1.0, 0.5, g, dt, (1.0, 0.5)) for g in RULE_GRADIENTS)  # dyadic weights: always
    assert not any(R.spec_holds(0.7, 0.3, g, torch.float32, (float(np.float32(0.7)), float(np.float32(0.3)))) for g in RULE_GRADIENTS)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("g_loss", RULE_GRADIENTS, ids=["third", "3.7", "twelfth"])
@pytest.mark.parametrize("w", RULE_WEIGHTS, ids=lambda w: "-".join(map(str, w)))
def test_speculation_stands_exactly_when_the_restated_rule_says_so(lib, step_case, w, g_loss, dtype):
    """Upstream gradients that are no powers of two: T(w_geom g) w_photo == T(w_photo g) w_geom decides (always true for the
    dyadic 1 / 0.5; false for 0.7 / 0.3 in fp32 at each of these gradients), sums[8] after the backward says what
    _spec_rule.spec_holds says of the pair the forward stored -- the weights rounded to the element type -- and on either
    route the gradients equal the fp64 oracle's."""
    T = np.float32 if dtype == torch.float32 else np.float64
    R.check_step(lib, step_case[dtype], w, g_loss, None, stored=(float(T(w[0])), float(T(w[2]))))


AUTOGRAD_WEIGHTS = [(0.7, 0.1, 0.3), (1.0, 0.0, 0.5), (1.0, 0.1, 0.0), (0.0, 0.1, 0.5), (0.0, 0.0, 0.5)]


@pytest.mark.parametrize("w", AUTOGRAD_WEIGHTS, ids=lambda w: "-".join(map(str, w)))
def test_single_node_step_at_other_and_zero_weights(on_sim, lib, monkeypatch, w):
    """compute_total_loss against the three reference-style calls plus the weighted sum, values and every gradient, with
    loss.backward() and (0.125 * loss).backward().  -c 0: r_hint = 0;
    -s 0: the smooth gradient rides as zeros; -p 0: no hint, the plain forward and ONE stand-alone smooth forward.  Where
    the step speculates, the workspace that reaches the backward still holds a standing speculation afterwards."""
    from scsfm_hip import config
    import loss_functions as LF
    B, H, W, n_ref, seed = R.CASE
    rides = w[0] != 0
    seen = []
    real_bwd = capi.photo_geometry_bwd

    def recording(*a, **k):
        seen.append(a[9])  # ws
        return real_bwd(*a, **k)

    z = lambda t: torch.zeros_like(t) if t.grad is None else t.grad.clone()

    def reference(c):
        ti, ris, K, td, rd, ps, pis = _leaves(B, H, W, n_ref, seed)
        photo, geom = LF.compute_photo_and_geometry_loss(ti, ris, K, td, rd, ps, pis, 1, 1, 1, 1, "zeros")
        smooth = LF.compute_smooth_loss(td, ti, rd, ris)
        loss = w[0] * photo + w[1] * smooth + w[2] * geom
        (c * loss).backward()
        return [float(v.detach()) for v in (loss, photo, smooth, geom)], [z(td[0])] + [z(r[0]) for r in rd] + [z(p) for p in ps + pis]

    def step(c):
        ti, ris, K, td, rd, ps, pis = _leaves(B, H, W, n_ref, seed)
        n0 = on_sim["smooth_fwd"]
        loss, photo, smooth, geom = LF.compute_total_loss(ti, ris, K, td, rd, ps, pis, 1, 1, 1, 1, "zeros", *w)
        # which route ran: the speculative forward carries the smooth loss unless -p 0 switches the speculation off
        assert on_sim["smooth_fwd"] - n0 == (0 if rides else 1), w
        del seen[:]
        (c * loss).backward()
        assert len(seen) == 1
        if rides:
            for j in range(2 * n_ref):
                s = R.sums_of(lib, seen[0], j, B, H, W)
                assert float(s[5]) != 0.0 and float(s[6]) != 0.0
                assert float(s[8]) == 1.0, (w, c, j, s[8:11].tolist())
        return [float(v.detach()) for v in (loss, photo, smooth, geom)], [z(td[0])] + [z(r[0]) for r in rd] + [z(p) for p in ps + pis]

    config.set_smooth_rides_along(True)
    monkeypatch.setattr(capi, "photo_geometry_bwd", recording)
    for c in (1.0, 0.125):
        # the reference-style calls speculate on the same weights (a user of the reference's loop with other -p / -c says
        # config.set_weight_hint(p, c)): both sides then take the same route to the gradients, which is
        # what the 1e-6 below presumes (across routes the fixed-point planes differ by more: the oracle judges those, above)
        config.set_weight_hint(w[0], w[2])
        try:
            v0, g0 = reference(c)
        finally:
            config.set_weight_hint(1.0, 0.5)  # the package default
        v1, g1 = step(c)
        for a, b in zip(v1, v0):
            assert abs(a - b) <= 1e-6 * abs(b), (w, c, v1, v0)
        for k, (a, b) in enumerate(zip(g1, g0)):
            assert float((a - b).abs().max()) <= 1e-6 * float(b.abs().max()), (w, c, k)
