"""Times frame-to-model tracking with a scale (scsfm_hip.similarity, libscsfm_sim3.so; reconstruct.py --refine-scale) against
the rigid tracker and records what the seventh degree of freedom does to the poses and to the model when the depth's scale
drifts.

    python tools/bench_similarity.py [--reps 15] [--out profiles/similarity_bench.json] [--dims 512 128 512] [--frames 64]

Timing.  tools/bench_tracking.py's protocol and maps: a model of the first eight generated frames of the "drive" scene at
256 x 832 in a 512 x 128 x 512 volume, cast from eight guesses; one similarity.align call of eight frames and ten
iterations against one tracking.align call on the same maps.  The two alternate in one process after a warm-up of each; a
sample is the time between two events round the call (its allocations included), the device idle before it.  Reported per
variant: median, minimum and maximum of --reps (at least 15) samples.  No time is gated: both calls are twenty launches
and are expected to be launch-bound and level.

Quality.  bench_tracking.py's generated world (one height field seen by 64 cameras; the chain is the true trajectory with
a known drift) with a drift of the depth's scale added: frame k's true depth is divided by 1 + 0.04 sin(0.45 k), the first
frame's by 1.  Recorded for pass two at the chained poses, with --refine-poses and with --refine-poses --refine-scale
(groups of 1): the mean and the last frame's translation and rotation error against the truth, reconstruct.py --render's
mean |pred - fused| / fused of the model fused that way (for the third mode with the scaled prediction, as the program
compares it), and for the third mode the error of the scales found and the frames whose scale was held throughout.

Not measured: a real sequence with trained nets; the kernels alone under a profiler; groups other than 1; other drifts.
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
from bench_tracking import BATCH, ITERATIONS, drifted, plain_pass, pose_errors, refined_pass, world_scene  # noqa: E402

SCALE_DRIFT = 0.04


def scaled_pass(vol, disp, images, c2w, K, max_depth, sink):
    """reconstruct.refine's loop with --refine-scale at groups of 1 -> (the refined poses [F, 3, 4], the scales [F])"""
    from reconstruct import relative_to
    from scsfm_hip import similarity
    refined, scales = c2w.clone(), torch.ones(len(c2w), dtype=torch.float64, device=c2w.device)
    vol.integrate(similarity.scaled_depth(disp[:1], scales[:1], True), images[:1], c2w[:1].contiguous(), K, is_disp=False,
                  max_depth=max_depth)
    for k in range(1, len(c2w)):
        idx = slice(k, k + 1)
        guess = relative_to(refined[k - 1], c2w[k - 1], c2w[idx])
        scale0 = scales[k - 1:k].clone()
        got = vol.track_scaled(disp[idx], guess, scale0, K, is_disp=True, max_depth=max_depth, iterations=ITERATIONS)
        kept = similarity.kept_guess(got.report)
        refined[idx] = torch.where(kept[:, None, None], guess, got.c2w)
        scales[idx] = torch.where(kept, scale0, got.scale)
        vol.integrate(similarity.scaled_depth(disp[idx], scales[idx], True), images[idx], refined[idx].contiguous(), K,
                      is_disp=False, max_depth=max_depth)
        sink.append(got.report)
    return refined, scales


def agreement(vol, pred, c2w, K, max_depth, min_weight=2.0):
    """reconstruct.py --render's figure for the predicted depths ``pred`` [F, H, W]: mean |pred - fused| / fused over the
    pixels with a hit and pred <= max_depth"""
    H, W = pred.shape[-2:]
    total, count, hits = 0.0, 0, 0
    for k in range(0, len(c2w), BATCH):
        got = vol.raycast(c2w[k:k + BATCH].contiguous(), K, (H, W), 0.0, max_depth + vol.trunc, min_weight=min_weight,
                          normals=False, colour=False, shade=False)
        p = pred[k:k + BATCH]
        hit = got.depth > 0
        both = hit & (p <= max_depth)
        ratio = (p.double() - got.depth.double()).abs() / got.depth.double()
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "similarity_bench.json"))
    args = ap.parse_args(argv)
    if args.reps < 15:
        raise SystemExit("--reps: at least 15")
    if not torch.cuda.is_available():
        raise SystemExit("bench_similarity.py needs a HIP device")
    from scsfm_hip import _lib, fusion, raycast, similarity, tracking
    _lib.get_fuse(), _lib.get_cast(), _lib.get_track(), _lib.get_sim3()  # (a missing library is an error before any timing)
    dev = torch.device("cuda")
    F, (H, W), dims = args.frames, args.size, tuple(args.dims)
    voxel = 16.0 / max(dims)
    origin = (-0.5 * dims[0] * voxel + 0.6, -0.5 * dims[1] * voxel, -1.0)
    disp, images, c2w, K, max_depth = scene(F, H, W, dev, "drive")

    # one align call of each library on the maps of a model of the first eight frames
    model = fusion.Volume(dims, origin, voxel, device=dev)
    model.integrate(disp[:BATCH], images[:BATCH], c2w[:BATCH].contiguous(), K, is_disp=True, max_depth=max_depth)
    guess = c2w[1:1 + BATCH].clone()
    guess[:, 0, 3] += 0.03
    cast = model.raycast(guess, K, (H, W), 0.0, max_depth + model.trunc, min_weight=1.0, colour=False, shade=False)
    ref_view = raycast.views(guess, K)
    frames = disp[1:1 + BATCH]
    trunc = model.trunc
    ones = torch.ones(BATCH, dtype=torch.float64, device=dev)
    del model
    kw = dict(is_disp=True, max_depth=max_depth, iterations=ITERATIONS, max_dist=trunc)
    variants = {"track_align_8_frames": lambda: tracking.align(frames, guess, K, ref_view, cast.depth, cast.normal, **kw),
                "sim3_align_8_frames": lambda: similarity.align(frames, guess, ones, K, ref_view, cast.depth, cast.normal,
                                                                **kw)}

    def timed(fn):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    got = variants["sim3_align_8_frames"]()
    rigid = variants["track_align_8_frames"]()
    statuses = sorted(set(got.report[:, :, 2].reshape(-1).tolist()))
    print(f"align: {BATCH} frames, {ITERATIONS} iterations, pairs at the last one "
          f"{[int(v) for v in got.report[:, -1, 0].tolist()]} (rigid {[int(v) for v in rigid.report[:, -1, 0].tolist()]}), "
          f"statuses {statuses}, scales {[round(v, 5) for v in got.scale.tolist()]}", flush=True)
    for fn in variants.values():
        timed(fn)
    runs = {k: [] for k in variants}
    for _ in range(args.reps):
        for k, fn in variants.items():
            runs[k].append(timed(fn))
    out = {k: stats(v) for k, v in runs.items()}
    for k, e in out.items():
        print(f"{k}: {e['median_ms']:.3f} ms ({e['min_ms']:.3f} .. {e['max_ms']:.3f})", flush=True)
    out["sim3_over_track_median"] = out["sim3_align_8_frames"]["median_ms"] / out["track_align_8_frames"]["median_ms"]
    out["sums_37_over_29"] = 37 / 29
    out["align_statuses"] = statuses

    # quality, on the scene that is one world, with a drift of the depth's scale
    del disp, images, c2w, frames, cast
    disp, images, truth, K, max_depth = world_scene(F, H, W, dev)
    factor = 1.0 + SCALE_DRIFT * torch.sin(0.45 * torch.arange(F, dtype=torch.float64, device=dev))
    disp = (disp * factor.float()[:, None, None, None]).contiguous()       # the depth divided by the factor
    chain = drifted(truth)
    vol = fusion.Volume(dims, origin, voxel, device=dev)
    quality = {}
    for name in ("chained", "refine_poses", "refine_poses_refine_scale"):
        vol.planes.zero_()
        reports, scales = [], None
        if name == "chained":
            plain_pass(vol, disp, images, chain, K, max_depth)
            poses = chain
        elif name == "refine_poses":
            poses = refined_pass(vol, disp, images, chain, K, 1, max_depth, reports)
        else:
            poses, scales = scaled_pass(vol, disp, images, chain, K, max_depth, reports)
        pred = 1.0 / disp[:, 0] if scales is None else similarity.scaled_depth(disp, scales, True)[:, 0]
        quality[name] = {**pose_errors(poses, truth), **agreement(vol, pred, poses, K, max_depth)}
        if reports:
            rep = torch.cat(reports)
            quality[name]["frames_that_kept_their_guess"] = int(((rep[:, :, 2] == 1) | (rep[:, :, 2] == 2)).all(1).sum())
            quality[name]["mean_pair_share"] = float(rep[:, -1, 0].mean()) / (H * W)
        if scales is not None:
            err = (scales - factor).abs()
            quality[name]["scale_error_mean"] = float(err.mean())
            quality[name]["scale_error_max"] = float(err.max())
            quality[name]["frames_whose_scale_was_held_throughout"] = int(similarity.held_scale(rep).sum())
            quality[name]["smallest_scale_pivot_ratio_of_a_solved_iteration"] = float(
                rep[:, :, 4][rep[:, :, 2] == 0].min()) if bool((rep[:, :, 2] == 0).any()) else float("nan")
        print(name, json.dumps(quality[name]), flush=True)
    result = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "dims": list(dims), "frames": F,
              "frame_size": [H, W], "iterations": ITERATIONS, "max_depth": max_depth, "max_dist": trunc,
              "min_scale_pivot": similarity.MIN_SCALE_PIVOT, **out,
              "quality_scene": {"drift_at_last_frame": {"x": 0.25, "yaw_rad": 0.03},
                                "depth_divided_by": "1 + 0.04 sin(0.45 k)", **quality},
              "not_measured": ["a real sequence with trained nets", "the kernels alone under a profiler",
                               "groups other than 1", "other drifts of the scale"]}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps({k: v for k, v in result.items() if k not in ("track_align_8_frames", "sim3_align_8_frames")}))


if __name__ == "__main__":
    main()
