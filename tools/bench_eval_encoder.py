"""Times the eval-mode forward of DispResNet(18), DispResNet(50) and PoseResNet(18) under torch.no_grad() at 256 x 832,
batches 1 and 4 (no dataset needed: seeded weights and inputs), with the encoder's fused eval-mode glue
(scsfm_hip.encoder_eval, libscsfm_enceval.so) against the ATen chain of the same commit.

    python tools/bench_eval_encoder.py [--reps 15] [--inner 10] [--out profiles/eval_encoder_bench.json]

  fused   the default: BatchNorm / ReLU / residual add / max-pool of the encoder through libscsfm_enceval.so
  torch   SCSFM_EVAL_TORCH=1: the same modules through ATen (BatchNorm, add, ReLU, max-pool as separate launches)
Both run in this process and alternate after a warm-up of each.  A sample is the host clock around --inner forwards
between two device synchronisations, divided by --inner; reported are the median, minimum and maximum of --reps (at least
15) samples, for the whole network and for its encoder alone, and the number of kernels one forward launches on each path
(counted by torch.profiler in a run of its own).  "fused_slower" is set where the fused path's fastest sample is slower
than the ATen chain's slowest (medians apart, spreads not overlapping): the rule by which the dispatch would become
opt-in.  The two paths' outputs are compared at 1e-4 of their scale.  Writes one JSON file.  Needs a HIP device."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sc-sfmlearner-release_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

H, W = 256, 832
BATCHES = (1, 4)
NETS = (("DispResNet", 18), ("DispResNet", 50), ("PoseResNet", 18))


def set_path(name):
    if name == "torch":
        os.environ["SCSFM_EVAL_TORCH"] = "1"
    else:
        os.environ.pop("SCSFM_EVAL_TORCH", None)


def count_kernels(fn):
    """kernels launched by one call of fn, as torch.profiler sees them (None and the reason where it cannot)"""
    try:
        from torch.profiler import ProfilerActivity, profile
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA
                and not e.name.lower().startswith(("memcpy", "memset")))
        return n, None
    except Exception as exc:  # the timings do not depend on the profiler
        return None, f"{type(exc).__name__}: {exc}"


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval_encoder_bench.json"))
    args = ap.parse_args(argv)
    if args.reps < 15:
        raise SystemExit("--reps: at least 15")
    if not torch.cuda.is_available():
        raise SystemExit("bench_eval_encoder.py needs a HIP device")
    import models
    from scsfm_hip import encoder_eval  # noqa: F401  (a missing library is an error before anything is timed)
    from scsfm_hip import _lib
    _lib.get_enceval()
    dev = torch.device("cuda")

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.inner):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / args.inner

    def stats(v):
        return {"median_ms": float(np.median(v)), "min_ms": float(np.min(v)), "max_ms": float(np.max(v)),
                "runs_ms": [round(float(x), 4) for x in v]}

    entries = []
    for kind, layers in NETS:
        torch.manual_seed(layers)
        net = getattr(models, kind)(layers, False).to(dev).eval()
        with torch.no_grad():  # running statistics as after training, not the initial 0 / 1
            for m in net.modules():
                if isinstance(m, torch.nn.BatchNorm2d):
                    m.running_mean.normal_(0, 0.1)
                    m.running_var.uniform_(0.5, 1.5)
        for batch in BATCHES:
            gen = torch.Generator(device=dev).manual_seed(batch)
            imgs = [torch.rand(batch, 3, H, W, device=dev, generator=gen) for _ in range(2)]
            enc_in = imgs[0] if kind == "DispResNet" else torch.cat(imgs, 1)

            @torch.no_grad()
            def whole():
                return net(imgs[0]) if kind == "DispResNet" else net(imgs[0], imgs[1])

            @torch.no_grad()
            def encoder():
                return net.encoder(enc_in)

            outs, kernels, note = {}, {}, None
            for path in ("fused", "torch"):  # (also the warm-up of both paths)
                set_path(path)
                for _ in range(3):
                    out = whole()
                    encoder()
                outs[path] = out.float().clone()
                kernels[path] = {}
                for what, fn in (("whole", whole), ("encoder", encoder)):
                    kernels[path][what], err = count_kernels(fn)
                    note = note or err
            scale = float(outs["torch"].abs().max())
            diff = float((outs["fused"] - outs["torch"]).abs().max())
            t = {(p, w): [] for p in ("fused", "torch") for w in ("whole", "encoder")}
            for _ in range(args.reps):
                for path in ("fused", "torch"):
                    set_path(path)
                    t[(path, "whole")].append(timed(whole))
                    t[(path, "encoder")].append(timed(encoder))
            set_path("fused")
            entry = {"net": f"{kind}({layers})", "batch": batch, "input": [H, W], "kernels_per_forward": kernels,
                     "max_abs_difference_of_the_outputs": diff, "output_scale": scale}
            if note:
                entry["kernel_count_note"] = note
            for what in ("whole", "encoder"):
                f, a = stats(t[("fused", what)]), stats(t[("torch", what)])
                entry[what] = {"fused": f, "torch": a, "ratio_torch_over_fused": a["median_ms"] / f["median_ms"],
                               "fused_slower": f["min_ms"] > a["max_ms"]}
            entries.append(entry)
            print(f"{entry['net']} B={batch}: whole {entry['whole']['fused']['median_ms']:.3f} ms fused / "
                  f"{entry['whole']['torch']['median_ms']:.3f} ms torch; encoder "
                  f"{entry['encoder']['fused']['median_ms']:.3f} / {entry['encoder']['torch']['median_ms']:.3f} ms; "
                  f"kernels {kernels['fused']} / {kernels['torch']}", flush=True)
            if not diff <= 1e-4 * scale:
                raise SystemExit(f"{entry['net']} B={batch}: the two paths differ by {diff:.3e} of {scale:.3e}")

    result = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "forwards_per_sample": args.inner,
              "any_fused_slower": any(e[w]["fused_slower"] for e in entries for w in ("whole", "encoder")),
              "entries": entries}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps({k: v for k, v in result.items() if k != "entries"}))


if __name__ == "__main__":
    main()
