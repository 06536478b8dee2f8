"""Times the one-launch Adam of scsfm_hip.optim (libscsfm_opt.so; train.py --optimizer hip) against torch.optim.Adam.

    python tools/bench_optimizer.py [--reps 15] [--out profiles/optimizer_bench.json] [--skip-e2e]

  step   optimizer.step() alone over the parameter lists train.py forms, DispResNet(18) + PoseResNet(18) and then
         DispResNet(50) + PoseResNet(18), every gradient present: this optimiser, torch's default (foreach) and torch's
         fused=True alternate in one process after a warm-up of all three.  A sample is the time between two events
         around --inner steps, the device idle before the first, divided by --inner -- so it holds the host's work per
         step too (the table, the foreach dispatch), as a training step does.  Reported: the median, minimum and maximum
         of --reps (at least 15) samples, and for this optimiser the bytes (28 per element: read p, g, m, v; write p, m, v)
         over the median as a share of the 8 TB/s HBM rate.
  e2e    a whole train_step at batch 12, 256 x 832, R18 + R18, --optimizer hip against torch, alternating, the
         parameters put back before every step.

"hip_slower" is set where this optimiser's fastest sample is slower than the other's slowest.  Writes one JSON file; an
existing "default_step_vs_parent" entry of that file (bench.py runs of this tree and of its parent, recorded by hand) is
kept.  Needs a HIP device."""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sc-sfmlearner-release_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

HBM_BYTES_PER_S = 8.0e12
BYTES_PER_ELEMENT = 28


def stats(v):
    return {"median_ms": float(np.median(v)), "min_ms": float(np.min(v)), "max_ms": float(np.max(v)),
            "runs_ms": [round(float(x), 4) for x in v]}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--inner", type=int, default=10, help="optimizer steps per sample (the end-to-end case: 1)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optimizer_bench.json"))
    ap.add_argument("--skip-e2e", action="store_true")
    args = ap.parse_args(argv)
    if args.reps < 15:
        raise SystemExit("--reps: at least 15")
    if not torch.cuda.is_available():
        raise SystemExit("bench_optimizer.py needs a HIP device")
    import models
    import train as T
    from scsfm_hip import _lib, optim, synth
    _lib.get_opt()  # (a missing library is an error before anything is timed)
    dev = torch.device("cuda")

    def timed(fn, inner):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / inner

    def make(name, groups):
        kw = dict(lr=1e-4, betas=(0.9, 0.999), weight_decay=0)
        if name == "hip":
            return optim.Adam(groups, **kw)
        return torch.optim.Adam(groups, fused=True, **kw) if name == "torch_fused" else torch.optim.Adam(groups, **kw)

    # ---- the step alone ---------------------------------------------------------------------------------------------------
    steps = []
    names = ("hip", "torch_foreach", "torch_fused")
    for layers in (18, 50):
        torch.manual_seed(0)
        nets = [models.DispResNet(layers, False), models.PoseResNet(18, False)]
        shapes = [[tuple(p.shape) for p in net.parameters() if p.requires_grad] for net in nets]
        gen = torch.Generator(device=dev).manual_seed(layers)
        opts, params = {}, {}
        for name in names:  # each optimiser on its own copy of the parameters, all with the same gradients' values
            groups = [{"params": [torch.nn.Parameter(torch.randn(s, device=dev, generator=gen) * 0.05) for s in group]}
                      for group in shapes]
            params[name] = [p for g in groups for p in g["params"]]
            for p in params[name]:
                p.grad = torch.randn(p.shape, device=dev, generator=gen) * 1e-3
            opts[name] = make(name, groups)
        for name in names:
            for _ in range(3):
                opts[name].step()
        t = {name: [] for name in names}
        for _ in range(args.reps):
            for name in names:
                t[name].append(timed(opts[name].step, args.inner))
        n = sum(p.numel() for p in params["hip"])
        entry = {"nets": f"DispResNet({layers}) + PoseResNet(18)", "tensors": len(params["hip"]), "elements": n,
                 **{name: stats(t[name]) for name in names}}
        entry["hip_bytes"] = n * BYTES_PER_ELEMENT
        entry["hip_share_of_hbm_rate"] = entry["hip_bytes"] / (entry["hip"]["median_ms"] * 1e-3) / HBM_BYTES_PER_S
        entry["hip_gb_per_s"] = entry["hip_bytes"] / (entry["hip"]["median_ms"] * 1e-3) / 1e9
        for other in names[1:]:
            entry[f"ratio_{other}_over_hip"] = entry[other]["median_ms"] / entry["hip"]["median_ms"]
        entry["hip_slower"] = any(entry["hip"]["min_ms"] > entry[o]["max_ms"] for o in names[1:])
        steps.append(entry)
        print(f"step {entry['nets']}: {entry['tensors']} tensors, {n / 1e6:.1f} M elements: hip "
              f"{entry['hip']['median_ms']:.4f} ms ({entry['hip_gb_per_s']:.0f} GB/s, "
              f"{100 * entry['hip_share_of_hbm_rate']:.0f} % of the HBM rate), foreach "
              f"{entry['torch_foreach']['median_ms']:.4f} ms, fused=True {entry['torch_fused']['median_ms']:.4f} ms"
              f"{'  HIP SLOWER' if entry['hip_slower'] else ''}", flush=True)
        del opts, params
        torch.cuda.empty_cache()

    # ---- a whole training step ------------------------------------------------------------------------------------------
    e2e = []
    if not args.skip_e2e:
        B, H, W = 12, 256, 832
        gen = torch.Generator().manual_seed(1234)
        mk = lambda: ((torch.rand(B, 3, H, W, generator=gen) - 0.45) / 0.225).to(dev)  # noqa: E731
        tgt, refs = mk(), [mk(), mk()]
        K = synth.intrinsics(np.random.default_rng(0), B, H, W, "kitti").to(dev)
        targs = argparse.Namespace(photo_loss_weight=1.0, smooth_loss_weight=0.1, geometry_consistency_weight=0.5,
                                   num_scales=1, with_ssim=1, with_mask=1, with_auto_mask=1, padding_mode="zeros", world=1,
                                   exact_mask_normalisation=False, channels_last=0)
        torch.manual_seed(0)
        disp_net, pose_net = models.DispResNet(18, False).to(dev).train(), models.PoseResNet(18, False).to(dev).train()
        groups = [{"params": [p for p in net.parameters() if p.requires_grad]} for net in (disp_net, pose_net)]
        trainable = [p for g in groups for p in g["params"]]
        start = [p.detach().clone() for p in trainable]
        opts = {name: make(name, [{"params": list(g["params"])} for g in groups]) for name in ("hip", "torch_foreach")}

        def step(name):
            with torch.no_grad():
                torch._foreach_copy_(trainable, start)
            return T.train_step(targs, disp_net, pose_net, opts[name], tgt, refs, K)

        for name in opts:
            for _ in range(3):
                step(name)
        t = {name: [] for name in opts}
        for _ in range(args.reps):
            for name in opts:
                t[name].append(timed(lambda: step(name), 1))
        entry = {"what": "train_step", "batch": B, "input": [H, W], "hip": stats(t["hip"]), "torch": stats(t["torch_foreach"])}
        entry["ratio_torch_over_hip"] = entry["torch"]["median_ms"] / entry["hip"]["median_ms"]
        entry["hip_slower"] = entry["hip"]["min_ms"] > entry["torch"]["max_ms"]
        e2e.append(entry)
        print(f"train_step: {entry['hip']['median_ms']:.2f} ms --optimizer hip / {entry['torch']['median_ms']:.2f} ms torch "
              f"(x {entry['ratio_torch_over_hip']:.3f}){'  HIP SLOWER' if entry['hip_slower'] else ''}", flush=True)

    result = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "steps_per_sample": args.inner,
              "hbm_bytes_per_s": HBM_BYTES_PER_S, "bytes_per_element": BYTES_PER_ELEMENT,
              "any_hip_slower": any(e["hip_slower"] for e in steps + e2e), "step": steps, "end_to_end": e2e}
    if os.path.exists(args.out):
        with open(args.out) as f:
            old = json.load(f)
        if "default_step_vs_parent" in old:
            result["default_step_vs_parent"] = old["default_step_vs_parent"]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps({k: v for k, v in result.items() if k not in ("step", "end_to_end")}))


if __name__ == "__main__":
    main()
