"""Times frame-to-model tracking (scsfm_hip.tracking, libscsfm_track.so; reconstruct.py --refine-poses) and records what it
does to the poses and to the model.

    python tools/bench_tracking.py [--reps 15] [--out profiles/tracking_bench.json] [--dims 512 128 512] [--frames 64]

Timing.  tools/bench_fusion.py's setup: the 64 generated frames of its "drive" scene at 256 x 832 and a 512 x 128 x 512
volume.  Pass two of reconstruct.py without the nets (the disparities are given): the plain pass integrates the frames in
batches of eight at the chained poses; the refined pass is reconstruct.refine's loop -- the first frame integrated, then per
group of --refine-group frames the guesses (torch, double), Volume.track (the brick mask, the cast, ten iterations) and
the integration at the refined poses -- at groups of 1 and of 8.  Beside them one tracking.align call of eight frames and
ten iterations against the same iterations written in torch operations (gather, masks, einsum, torch.linalg.solve) on the
same maps.  All variants alternate in one process after a warm-up of each; a sample is the time between two events round
the call (its allocations included), the device idle before it and the volume cleared outside the events.  Reported per
variant: median, minimum and maximum of --reps (at least 15) samples.

Quality.  The drive scene's frames are not views of one world, so the poses have no truth there.  The quality scene is
one: the height field z = 3 + 0.8 sin(0.7 x) cos(0.9 y) + 0.25 y seen by 64 cameras that move forward and turn; every
frame's depth is the ray's intersection with it (a fixed-point iteration in float64).  The chain is the true trajectory
with a known drift added, growing linearly to 0.25 in x and 0.03 rad of yaw at the last frame.  Recorded for the chained
poses and for the poses refined at groups of 1 and 8: the mean and the last frame's translation and rotation error against
the truth, and reconstruct.py --render's mean |pred - fused| / fused of the model fused at those poses.

Not measured: a real sequence with trained nets; the kernels alone under a profiler; group sizes other than 1 and 8.
Writes one JSON file.  Needs a HIP device."""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sc-sfmlearner-release_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench_fusion import scene, stats  # noqa: E402

ITERATIONS = 10
BATCH = 8


def refined_pass(vol, disp, images, c2w, K, group, max_depth, sink=None):
    """reconstruct.refine's loop on given disparities -> the refined poses [F, 3, 4]"""
    from reconstruct import relative_to
    from scsfm_hip import tracking
    refined = c2w.clone()
    vol.integrate(disp[:1], images[:1], c2w[:1].contiguous(), K, is_disp=True, max_depth=max_depth)
    for k in range(1, len(c2w), group):
        idx = slice(k, min(k + group, len(c2w)))
        guess = relative_to(refined[k - 1], c2w[k - 1], c2w[idx])
        got = vol.track(disp[idx], guess, K, is_disp=True, max_depth=max_depth, iterations=ITERATIONS)
        poses = torch.where(tracking.kept_guess(got.report)[:, None, None], guess, got.c2w)
        vol.integrate(disp[idx], images[idx], poses, K, is_disp=True, max_depth=max_depth)
        refined[idx] = poses
        if sink is not None:
            sink.append(got.report)
    return refined


def plain_pass(vol, disp, images, c2w, K, max_depth):
    for k in range(0, len(c2w), BATCH):
        vol.integrate(disp[k:k + BATCH], images[k:k + BATCH], c2w[k:k + BATCH].contiguous(), K, is_disp=True,
                      max_depth=max_depth)


def quat_matrix(q):
    w, x, y, z = q.unbind(-1)
    return torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                        2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                        2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], -1).reshape(-1, 3, 3)


def torch_align(disp, guess, K, ref_view, M, N, max_depth, max_dist, iterations, min_pairs=64):
    """the header's iteration in torch operations (the pair in float32, the sums and the solve in float64; the order of
    the sums is torch's) -> c2w [V, 3, 4].  The state is the matrix itself, re-orthonormalised through the same rational
    update of a quaternion-free form: R <- dR R with dR the matrix of normalise(1, w / 2)."""
    V, H, W = M.shape
    dev = M.device
    d = 1.0 / disp.reshape(V, -1)
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    i = torch.arange(H * W, device=dev)
    dx, dy = ((i % W).float() - cx) / fx, ((i // W).float() - cy) / fy
    q = torch.stack([dx * d, dy * d, d], -1)                                    # [V, P, 3]
    Rr, cr = ref_view[:, :9].reshape(V, 3, 3), ref_view[:, 9:12]
    R, c = guess[:, :, :3].clone(), guess[:, :, 3].clone()
    Mf, Nf = M.reshape(V, -1), N.reshape(V, 3, -1)
    rows = torch.arange(V, device=dev)[:, None]
    for _ in range(iterations):
        u = torch.einsum("vij,vpj->vpi", R.float(), q)
        p = u + c.float()[:, None]
        e = torch.einsum("vji,vpj->vpi", Rr, p - cr[:, None])
        z = e[..., 2]
        a, b = fx * e[..., 0] / z + cx + 0.5, fy * e[..., 1] / z + cy + 0.5
        ok = (d > 0) & (d <= max_depth) & (z > 0) & (a >= 0) & (a < W) & (b >= 0) & (b < H)
        at = torch.where(ok, b, torch.zeros_like(b)).long() * W + torch.where(ok, a, torch.zeros_like(a)).long()
        s = Mf[rows, at]
        n = Nf[rows[:, :, None], torch.arange(3, device=dev)[None, None], at[:, :, None]]   # [V, P, 3]
        w = torch.einsum("vij,vpj->vpi", Rr, torch.stack([((at % W).float() - cx) / fx, ((at // W).float() - cy) / fy,
                                                            torch.ones_like(s)], -1))
        m = cr[:, None] + s[..., None] * w
        delta = p - m
        ok &= (s > 0) & ((n * n).sum(-1) > 0) & ((delta * delta).sum(-1) <= max_dist * max_dist) & ((n * u).sum(-1) < 0)
        r = (n * delta).sum(-1)
        J = torch.cat([n, torch.cross(u, n, dim=-1)], -1).double()
        J = torch.where(ok[..., None], J, torch.zeros_like(J))
        r = torch.where(ok, r.double(), torch.zeros_like(r, dtype=torch.float64))
        Hm, g = torch.einsum("vpi,vpj->vij", J, J), torch.einsum("vpi,vp->vi", J, r)
        good = ok.sum(1) >= min_pairs
        Hm = torch.where(good[:, None, None], Hm, torch.eye(6, dtype=torch.float64, device=dev))
        x = torch.linalg.solve(Hm, -g[..., None])[..., 0] * good[:, None]
        h = 0.5 * x[:, 3:]
        dq = torch.cat([torch.ones_like(h[:, :1]), h], 1)
        R = quat_matrix(dq / dq.norm(dim=1, keepdim=True)) @ R
        c = c + x[:, :3]
    return torch.cat([R, c[:, :, None]], 2)


def world_scene(F, H, W, dev):
    """the quality scene -> disparity [F, 1, H, W], images, the true poses float64 [F, 3, 4], K, max_depth"""
    _, images, _, K, max_depth = scene(F, H, W, dev, "drive")
    Kc = K.double()
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float64, device=dev),
                            torch.arange(W, dtype=torch.float64, device=dev), indexing="ij")
    ray = torch.stack([(xx - Kc[0, 2]) / Kc[0, 0], (yy - Kc[1, 2]) / Kc[1, 1], torch.ones_like(xx)], -1)
    c2w = np.zeros((F, 3, 4))
    depth = []
    for k in range(F):
        a = 0.004 * k
        c2w[k, :, :3] = [[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]
        c2w[k, :, 3] = [0.02 * k, 0.0, 0.01 * k]
        w = ray @ torch.from_numpy(c2w[k, :, :3]).to(dev).T
        c = c2w[k, :, 3]
        d = torch.full((H, W), 3.0, dtype=torch.float64, device=dev)
        for _ in range(80):   # z = g(x, y) along the ray: a contraction, the slopes of g being below 1 / |w_xy / w_z|
            x, y = c[0] + d * w[..., 0], c[1] + d * w[..., 1]
            d = (3.0 + 0.8 * torch.sin(0.7 * x) * torch.cos(0.9 * y) + 0.25 * y - c[2]) / w[..., 2]
        depth.append(d)
    disp = (1.0 / torch.stack(depth)).float().unsqueeze(1).contiguous()
    return disp, images, torch.from_numpy(c2w).to(dev), K, max_depth


def drifted(c2w):
    """the true trajectory with the known drift: k / (F - 1) of 0.25 in x and of 0.03 rad of yaw"""
    out = c2w.clone()
    F = len(c2w)
    for k in range(F):
        a = 0.03 * k / (F - 1)
        Ry = torch.tensor([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]], dtype=torch.float64,
                          device=c2w.device)
        out[k, :, :3] = Ry @ c2w[k, :, :3]
        out[k, 0, 3] += 0.25 * k / (F - 1)
    return out


def pose_errors(c2w, truth):
    dt = (c2w[:, :, 3] - truth[:, :, 3]).norm(dim=1)
    R = c2w[:, :, :3] @ truth[:, :, :3].transpose(1, 2)
    ang = torch.acos(((R.diagonal(dim1=1, dim2=2).sum(1) - 1) / 2).clamp(-1, 1))
    return {"translation_mean": float(dt.mean()), "translation_last": float(dt[-1]), "rotation_mean_rad": float(ang.mean()),
            "rotation_last_rad": float(ang[-1])}


def agreement(vol, disp, c2w, K, max_depth, min_weight=2.0):
    """reconstruct.py --render's figure: mean |pred - fused| / fused over the pixels with a hit and pred <= max_depth"""
    H, W = disp.shape[-2:]
    total, count, hits = 0.0, 0, 0
    for k in range(0, len(c2w), BATCH):
        got = vol.raycast(c2w[k:k + BATCH].contiguous(), K, (H, W), 0.0, max_depth + vol.trunc, min_weight=min_weight,
                          normals=False, colour=False, shade=False)
        pred = 1.0 / disp[k:k + BATCH, 0]
        hit = got.depth > 0
        both = hit & (pred <= max_depth)
        ratio = (pred.double() - got.depth.double()).abs() / got.depth.double()
        total += float(torch.where(both, ratio, torch.zeros_like(ratio)).sum())
        count += int(both.sum())
        hits += int(hit.sum())
    return {"mean_rel_depth_difference": total / count if count else float("nan"), "pixels": count,
            "share_of_pixels_with_a_hit": hits / (len(c2w) * H * W)}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--dims", type=int, nargs=3, default=[512, 128, 512])
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--size", type=int, nargs=2, default=[256, 832])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tracking_bench.json"))
    args = ap.parse_args(argv)
    if args.reps < 15:
        raise SystemExit("--reps: at least 15")
    if not torch.cuda.is_available():
        raise SystemExit("bench_tracking.py needs a HIP device")
    from scsfm_hip import _lib, fusion, raycast, tracking
    _lib.get_fuse(), _lib.get_cast(), _lib.get_track()  # (a missing library is an error before anything is timed)
    dev = torch.device("cuda")
    F, (H, W), dims = args.frames, args.size, tuple(args.dims)
    voxel = 16.0 / max(dims)
    origin = (-0.5 * dims[0] * voxel + 0.6, -0.5 * dims[1] * voxel, -1.0)
    vol = fusion.Volume(dims, origin, voxel, device=dev)
    disp, images, c2w, K, max_depth = scene(F, H, W, dev, "drive")

    def timed(fn):
        vol.planes.zero_()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    # one align call and the same iterations in torch, on the maps of a model of the first eight frames
    model = fusion.Volume(dims, origin, voxel, device=dev)
    model.integrate(disp[:BATCH], images[:BATCH], c2w[:BATCH].contiguous(), K, is_disp=True, max_depth=max_depth)
    guess = c2w[1:1 + BATCH].clone()
    guess[:, 0, 3] += 0.03
    cast = model.raycast(guess, K, (H, W), 0.0, max_depth + model.trunc, min_weight=1.0, colour=False, shade=False)
    ref_view = raycast.views(guess, K)
    frames = disp[1:1 + BATCH]
    del model

    def align():
        return tracking.align(frames, guess, K, ref_view, cast.depth, cast.normal, is_disp=True, max_depth=max_depth,
                              iterations=ITERATIONS, max_dist=vol.trunc)

    def in_torch():
        return torch_align(frames, guess, K, ref_view, cast.depth, cast.normal, max_depth, vol.trunc, ITERATIONS)

    got = align()
    try:
        other = in_torch()
        torch_error = None
        difference = float((other - got.c2w).abs().max())
    except RuntimeError as e:   # (a torch build without a device solver: the baseline is then named as not measured)
        torch_error, difference = str(e).splitlines()[0], None
    print(f"align: {BATCH} frames, {ITERATIONS} iterations, pairs at the last one "
          f"{[int(v) for v in got.report[:, -1, 0].tolist()]}, statuses {sorted(set(got.report[:, :, 2].reshape(-1).tolist()))}; "
          f"largest |torch - hip| of the poses {difference}", flush=True)

    variants = {"plain_pass_two": lambda: plain_pass(vol, disp, images, c2w, K, max_depth),
                "refined_group_1": lambda: refined_pass(vol, disp, images, c2w, K, 1, max_depth),
                "refined_group_8": lambda: refined_pass(vol, disp, images, c2w, K, 8, max_depth),
                "align_8_frames": align}
    if torch_error is None:
        variants["align_8_frames_torch"] = in_torch
    for fn in variants.values():
        timed(fn)
    runs = {k: [] for k in variants}
    for _ in range(args.reps):
        for k, fn in variants.items():
            runs[k].append(timed(fn))
    out = {k: stats(v) for k, v in runs.items()}
    for k, e in out.items():
        print(f"{k}: {e['median_ms']:.3f} ms ({e['min_ms']:.3f} .. {e['max_ms']:.3f})", flush=True)
    for k in ("refined_group_1", "refined_group_8"):
        out[k]["ms_per_tracked_frame_over_plain"] = (out[k]["median_ms"] - out["plain_pass_two"]["median_ms"]) / (F - 1)
    out["align_8_frames"]["ms_per_frame_and_iteration"] = out["align_8_frames"]["median_ms"] / (BATCH * ITERATIONS)

    # quality, on the scene that is one world
    del disp, images, c2w
    disp, images, truth, K, max_depth = world_scene(F, H, W, dev)
    chain = drifted(truth)
    quality = {}
    for name, group in (("chained", None), ("refined_group_1", 1), ("refined_group_8", 8)):
        vol.planes.zero_()
        reports = []
        if group is None:
            plain_pass(vol, disp, images, chain, K, max_depth)
            poses = chain
        else:
            poses = refined_pass(vol, disp, images, chain, K, group, max_depth, reports)
        quality[name] = {**pose_errors(poses, truth), **agreement(vol, disp, poses, K, max_depth)}
        if reports:
            rep = torch.cat(reports)
            quality[name]["frames_that_kept_their_guess"] = int(tracking.kept_guess(rep).sum())
            quality[name]["mean_pair_share"] = float(rep[:, -1, 0].mean()) / (H * W)
            ok = rep[:, :, 0] > 0
            rms = torch.sqrt(rep[:, :, 1] / rep[:, :, 0].clamp(min=1))
            quality[name]["mean_rms_first"] = float(rms[:, 0][ok[:, 0]].mean()) if bool(ok[:, 0].any()) else float("nan")
            quality[name]["mean_rms_last"] = float(rms[:, -1][ok[:, -1]].mean()) if bool(ok[:, -1].any()) else float("nan")
        print(name, json.dumps(quality[name]), flush=True)
    result = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "dims": list(dims), "frames": F,
              "frame_size": [H, W], "iterations": ITERATIONS, "max_depth": max_depth, "max_dist": vol.trunc,
              "align_torch_error": torch_error, "align_largest_pose_difference_torch_vs_hip": difference, **out,
              "quality_scene": {"drift_at_last_frame": {"x": 0.25, "yaw_rad": 0.03}, **quality},
              "not_measured": ["a real sequence with trained nets", "the kernels alone under a profiler",
                               "group sizes other than 1 and 8"]}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps({k: v for k, v in result.items() if k not in out}))


if __name__ == "__main__":
    main()
