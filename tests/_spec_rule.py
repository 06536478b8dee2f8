"""When does the speculative forward of the one-node step (ops.StepLoss -> scsfm_pairs_fwd_step) stand?  The rule the
kernels apply (csrc/scsfm_pair.hip: spec_valid on what pair_finalize_kernel stored and scsfm_step_weights formed), restated
once in numpy, and what the simulator tests and their hardware twins (tests/test_gpu_parity.py) share: the case, its fp64
oracle, StepLoss's sequence of library calls and the judgement of the gradients."""
import functools

import numpy as np
import torch

from _util import assert_close_frac

POSE_RTOL = 1.5e-2  # tests/test_hostsim_kernels.py, tests/test_gpu_parity.py
CASE = (4, 72, 100, 1, 41)  # B, H, W, references, seed: both gates of both pair-directions are open


def spec_holds(w_photo, w_geom, g_loss, dtype, stored):
    """The backward lets the speculative forward's results stand (open gates): the upstream gradients of the two terms are
    T(T(w) * T(g_loss)) (step_weights_kernel), ``stored`` = (sums[9], sums[10]) is what the forward speculated on, and the
    check multiplies them as doubles."""
    T = {torch.float32: np.float32, torch.float64: np.float64}.get(dtype, dtype)
    gp = T(T(w_photo) * T(g_loss))
    gg = T(T(w_geom) * T(g_loss))
    return bool(np.float64(gg) * np.float64(stored[0]) == np.float64(gp) * np.float64(stored[1]))


def sums_of(lib, ws, pair, B, H, W):
    """double[16] of pair-direction ``pair`` in the workspace of a SPECULATIVE photo_geometry_fwd (csrc/scsfm_common.h:
    PairWs -- the B constants slots of 256 bytes come first; the gbuf planes follow each pair's workspace).  [5], [6]: the
    photo / geometry gates' coefficients (0 = closed); [8]: the speculation stands; [9], [10]: the weights it assumed."""
    from scsfm_hip import capi
    ws_bytes, scratch_bytes, _ = capi._sizes(lib, B, H, W)
    stride = ws_bytes + scratch_bytes
    off = pair * stride + 256 * B
    return ws[off:off + 128].view(torch.float64)


def inputs(dtype, device="cpu"):
    """(tgt_img, K, ref_imgs, tgt_depths, ref_depths, poses, poses_inv) of CASE."""
    from scsfm_hip import synth
    B, H, W, n_ref, seed = CASE
    d = synth.make_batch(B, H, W, n_ref=n_ref, seed=seed, depth="smooth")
    c = lambda t: t.to(device=device, dtype=dtype).contiguous()
    return (c(d["tgt_img"]), c(d["intrinsics"]), [c(r) for r in d["ref_imgs"]], [c(d["tgt_depth"][0])],
            [[c(r[0])] for r in d["ref_depths"]], [c(p) for p in d["poses"]], [c(p) for p in d["poses_inv"]])


@functools.lru_cache(maxsize=1)
def oracle_terms():
    """fp64 oracle on the CPU, once: the values of (photo, smooth, geometry) of CASE with SSIM + mask + auto-mask and each
    term's gradients, in the order [tgt depth, ref depths..., poses..., poses_inv...]."""
    from oracle import scsfm_oracle as O
    ti, K, ris, tds, rds, ps, pis = inputs(torch.float64)
    lf = lambda t: t.clone().requires_grad_(True)
    td, rd, pp, pi = [lf(t) for t in tds], [[lf(r[0])] for r in rds], [lf(p) for p in ps], [lf(p) for p in pis]
    photo, geom = O.photo_and_geometry_loss(ti, ris, K, td, rd, pp, pi, 1, 1, 1, 1, "zeros")
    smooth = O.smooth_loss(td, ti, rd, ris)
    leaves = td + [r[0] for r in rd] + pp + pi
    z = lambda g, t: torch.zeros_like(t) if g is None else g
    grads = [[z(g, t) for g, t in zip(torch.autograd.grad(term, leaves, retain_graph=True, allow_unused=True), leaves)]
             for term in (photo, smooth, geom)]
    return [float(v.detach()) for v in (photo, smooth, geom)], grads


def oracle_gradients(w, g_loss):
    """d [g_loss * (w[0] photo + w[1] smooth + w[2] geometry)] / d every leaf, fp64."""
    _, (gp, gs, gg) = oracle_terms()
    return [g_loss * (w[0] * a + w[1] * b + w[2] * c) for a, b, c in zip(gp, gs, gg)]


def step_sequence(lib, x, w, g_loss):
    """The library calls ops.StepLoss makes for one step with the weights ``w`` = (w_photo, w_smooth, w_geom) and the upstream
    gradient ``g_loss`` -> (out[4], gradients in oracle_terms' order, the pairs' workspace after the backward)."""
    from scsfm_hip import capi
    ti, K, ris, tds, rds, ps, pis = x
    fl = capi.make_flags(1, 1, 1, "zeros")
    hint = (float(np.float32(w[0])), float(np.float32(w[2])))
    _, _, _, ws, _, sws, out = capi.photo_geometry_fwd(lib, fl, ti, K, ris, tds, rds, ps, pis, hint=hint, smooth=True,
                                                       keep_edges=True, step=w)
    g = torch.tensor([g_loss], dtype=ti.dtype, device=ti.device)
    gw = capi.step_weights(lib, g, *w)
    g_td, g_rd, g_p, g_pi = capi.photo_geometry_bwd(lib, fl, ti, K, ris, tds, rds, ps, pis, ws, gw[0:1], gw[1:2],
                                                    smooth=(sws, gw[2:3]))
    return out, [g_td[0]] + [r[0] for r in g_rd] + list(g_p) + list(g_pi), ws


def judge_gradients(got, want, dtype, what=""):
    """fp64 kernels: 1e-10 of the tensor's scale (tests/test_hostsim_kernels.py, every fp64 comparison with the oracle).  fp32:
    the judgement of test_total_loss_fp32_matches_reference_goldens and tests/test_gpu_parity.py::_scale_close -- depth
    gradients entry-wise at 0.2 % of the map's scale with 0.2 % of the entries set aside for flipped gates, pose gradients
    at POSE_RTOL of the tensor's scale."""
    for k, (a, b) in enumerate(zip(got, want)):
        a, b = a.detach().cpu().double(), b.double()
        scale = float(b.abs().max())
        if dtype == torch.float64:
            assert float((a - b).abs().max()) < 1e-10 * (scale + 1e-300), (what, k)
        elif b.dim() == 4:
            assert_close_frac(a.numpy(), b.numpy(), atol=2e-3 * scale, rtol=1e-3, max_bad_frac=2e-3, what=f"{what} map {k}")
        else:
            assert_close_frac(a.numpy(), b.numpy(), atol=POSE_RTOL * scale, what=f"{what} pose {k}")


def check_step(lib, x, w, g_loss, want_held, stored=None):
    """One step through step_sequence: gates open, what the forward stored, whether the speculation stood after the
    backward (``want_held``: True / False, or None = whatever spec_holds says of the stored pair), and the gradients
    against the fp64 oracle on either route.  -> the list of sums[8] per pair-direction."""
    B, H, W, n_ref, _ = CASE
    dtype = x[0].dtype
    out, grads, ws = step_sequence(lib, x, w, g_loss)
    held = []
    for j in range(2 * n_ref):
        s = sums_of(lib, ws, j, B, H, W).cpu()
        assert float(s[5]) != 0.0 and float(s[6]) != 0.0, "a gate is closed: the check would be vacuous"
        got = (float(s[9]), float(s[10]))
        if stored is not None:
            assert got == stored, (w, got, stored)
        want = spec_holds(w[0], w[2], g_loss, dtype, got) if want_held is None else want_held
        assert float(s[8]) == (1.0 if want else 0.0), (w, g_loss, j, float(s[8]), got)
        held.append(float(s[8]))
    vals, _ = oracle_terms()
    tol = 1e-5 if dtype == torch.float32 else 1e-10
    o = out.cpu().double()
    assert abs(float(o[1]) - vals[0]) <= tol and abs(float(o[2]) - vals[1]) <= tol and abs(float(o[3]) - vals[2]) <= tol
    assert abs(float(o[0]) - (w[0] * vals[0] + w[1] * vals[1] + w[2] * vals[2])) <= tol * (abs(w[0]) + abs(w[1]) + abs(w[2]))
    judge_gradients(grads, oracle_gradients(w, g_loss), dtype, what=f"w={w} g={g_loss}")
    return held
