"""Times fine-tuning with frozen BatchNorm statistics (train.py --freeze-bn): the fused path of scsfm_hip.encoder_frozen
(forward libscsfm_enceval.so, backward libscsfm_fbn.so) against the ATen chain through the same frozen modules, which is
what the parent commit would run for them.

    python tools/bench_frozen_bn.py [--reps 15] [--out profiles/frozen_bn_bench.json] [--skip-e2e]

  fused   the default
  torch   SCSFM_FROZEN_TORCH=1: BatchNorm, add, ReLU and their backward launches by ATen
Both run in this process and alternate after a warm-up of every shape on both paths.  A sample is the time between two
events around --inner repetitions, the device idle before the first, divided by --inner; reported are the median,
minimum and maximum of --reps (at least 15) samples.

  sites   forward plus backward of one site (a convolution's output through BatchNorm [+ identity] [+ ReLU]) at the five
          stage shapes of configs[1] (batch 12, 256 x 832), modes 0 / 1 / 2, with gamma and beta training (stats) and held
          (all); the bytes the fused pair of launches moves (forward 8 / 8 / 12 per element, backward 8 / 12 / 16, plus 4
          with parameter gradients) and the share of the 8 TB/s HBM rate that makes
  e2e     one forward plus backward of ResnetEncoder(18), and one whole train_step at configs[1], frozen-fused against
          frozen-ATen, and beside both the ordinary training-mode step (batch statistics) for orientation

"fused_slower" is set where the fused path's fastest sample is slower than the ATen chain's slowest (medians apart,
spreads not overlapping): the rule by which a class of calls is routed to ATen -- as the form without a ReLU (mode 0, the
down-sample branch) is by scsfm_hip.encoder_frozen.applies, which the end-to-end figures include.  Writes one JSON file; an existing
"default_step_vs_parent" entry of that file (bench.py runs of this tree and of its parent, recorded by hand) is kept.
Needs a HIP device."""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sc-sfmlearner-release_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

STAGE_SHAPES = [(12, 64, 128, 416), (12, 64, 64, 208), (12, 128, 32, 104), (12, 256, 16, 52), (12, 512, 8, 26)]
HBM_BYTES_PER_S = 8.0e12
FWD_BYTES = {0: 8, 1: 8, 2: 12}
BWD_BYTES = {0: 8, 1: 12, 2: 16}


def set_path(name):
    if name == "torch":
        os.environ["SCSFM_FROZEN_TORCH"] = "1"
    else:
        os.environ.pop("SCSFM_FROZEN_TORCH", None)


def stats(v):
    return {"median_ms": float(np.median(v)), "min_ms": float(np.min(v)), "max_ms": float(np.max(v)),
            "runs_ms": [round(float(x), 4) for x in v]}


def compare(t):
    f, a = stats(t["fused"]), stats(t["torch"])
    return {"fused": f, "torch": a, "ratio_torch_over_fused": a["median_ms"] / f["median_ms"],
            "fused_slower": f["min_ms"] > a["max_ms"]}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--inner", type=int, default=10, help="repetitions of a site per sample (the end-to-end cases: 1)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frozen_bn_bench.json"))
    ap.add_argument("--skip-e2e", action="store_true")
    args = ap.parse_args(argv)
    if args.reps < 15:
        raise SystemExit("--reps: at least 15")
    if not torch.cuda.is_available():
        raise SystemExit("bench_frozen_bn.py needs a HIP device")
    import torch.nn as nn

    import models
    import train as T
    from models.resnet_encoder import ResnetEncoder, _bn_act
    from scsfm_hip import _lib, encoder_frozen as EF, synth
    _lib.get_enceval(), _lib.get_fbn()  # (a missing library is an error before anything is timed)
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

    def alternate(fn, inner):
        t = {"fused": [], "torch": []}
        for _ in range(args.reps):
            for path in ("fused", "torch"):
                set_path(path)
                t[path].append(timed(fn, inner))
        set_path("fused")
        return t

    # ---- one site ---------------------------------------------------------------------------------------------------------
    relu = nn.ReLU(inplace=True)
    cases = []
    for shape in STAGE_SHAPES:
        gen = torch.Generator(device=dev).manual_seed(sum(shape))
        B, C, H, W = shape
        x = torch.randn(shape, device=dev, generator=gen).requires_grad_()
        identity = torch.randn(shape, device=dev, generator=gen).requires_grad_()
        g = torch.randn(shape, device=dev, generator=gen)
        for affine in (False, True):
            bn = nn.BatchNorm2d(C).to(dev)
            with torch.no_grad():
                bn.running_mean.normal_(0, 0.1)
                bn.running_var.uniform_(0.5, 1.5)
                bn.weight.uniform_(0.5, 1.5)
                bn.bias.normal_(0, 0.1)
            EF.freeze(bn, affine=affine)
            leaves = [x, identity] + ([] if affine else [bn.weight, bn.bias])
            for mode in (0, 1, 2):
                def site(bn=bn, mode=mode, leaves=leaves, x=x, identity=identity, g=g):
                    # (the fused op by name: the dispatch leaves mode 0 to ATen, and this is the measurement behind that)
                    if EF.enabled():
                        y = EF.bn_act(x, bn, identity if mode == 2 else None, relu=mode != 0)
                    else:
                        y = _bn_act(x, bn, relu if mode else None, identity if mode == 2 else None)
                    return torch.autograd.grad(y, [t for t in leaves if mode == 2 or t is not identity], g)
                cases.append((shape, mode, affine, site))
    outs = {}
    for path in ("fused", "torch"):  # the warm-up of every shape on both paths; the two paths' gradients are compared
        set_path(path)
        for k, (_, _, _, site) in enumerate(cases):
            for _ in range(3):
                outs[(path, k)] = site()
    sites = []
    for k, (shape, mode, affine, site) in enumerate(cases):
        for a, b in zip(outs[("fused", k)], outs[("torch", k)]):
            if not float((a - b).abs().max()) <= 1e-4 * float(b.abs().max()):
                raise SystemExit(f"{shape} mode {mode}: the two paths' gradients differ")
        entry = {"shape": list(shape), "mode": mode, "parameter_gradients": not affine, **compare(alternate(site, args.inner))}
        n = shape[0] * shape[1] * shape[2] * shape[3]
        entry["fused_bytes"] = n * (FWD_BYTES[mode] + BWD_BYTES[mode] + (0 if affine else 4))
        entry["fused_share_of_hbm_rate"] = entry["fused_bytes"] / (entry["fused"]["median_ms"] * 1e-3) / HBM_BYTES_PER_S
        sites.append(entry)
        print(f"site {shape} mode {mode} {'stats' if not affine else 'all  '}: {entry['fused']['median_ms']:.4f} ms fused / "
              f"{entry['torch']['median_ms']:.4f} ms torch (x {entry['ratio_torch_over_fused']:.2f}), "
              f"{100 * entry['fused_share_of_hbm_rate']:.0f} % of the HBM rate"
              f"{'  FUSED SLOWER' if entry['fused_slower'] else ''}", flush=True)
    del outs, cases

    # ---- end to end ---------------------------------------------------------------------------------------------------------
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

        def randomise(net):
            with torch.no_grad():
                for m in net.modules():
                    if isinstance(m, nn.BatchNorm2d):
                        m.running_mean.normal_(0, 0.1)
                        m.running_var.uniform_(0.5, 1.5)

        for mode in ("off", "stats", "all"):
            torch.manual_seed(0)
            enc = ResnetEncoder(18, False).to(dev)
            disp_net, pose_net = models.DispResNet(18, False).to(dev), models.PoseResNet(18, False).to(dev)
            for net in (enc, disp_net, pose_net):
                randomise(net)
                if mode != "off":
                    EF.freeze(net, affine=mode == "all")
                net.train()
            enc_params = [p for p in enc.parameters() if p.requires_grad]
            groups = [{"params": [p for p in net.parameters() if p.requires_grad]} for net in (disp_net, pose_net)]
            opt = torch.optim.Adam(groups, lr=1e-4, betas=(0.9, 0.999))
            trainable = [p for grp in groups for p in grp["params"]]
            start = [p.detach().clone() for p in trainable]

            def encoder():
                return torch.autograd.grad(sum(f.mean() for f in enc(tgt)), enc_params)

            def step():
                with torch.no_grad():
                    torch._foreach_copy_(trainable, start)
                return T.train_step(targs, disp_net, pose_net, opt, tgt, refs, K)

            for what, fn in (("encoder forward + backward", encoder), ("train_step", step)):
                paths = ("fused",) if mode == "off" else ("fused", "torch")
                for path in paths:
                    set_path(path)
                    for _ in range(3):
                        fn()
                if mode == "off":
                    entry = {"what": what, "freeze_bn": mode, "batch": B, "input": [H, W],
                             "training_mode": stats([timed(fn, 1) for _ in range(args.reps)])}
                    print(f"{what} --freeze-bn off: {entry['training_mode']['median_ms']:.2f} ms", flush=True)
                else:
                    entry = {"what": what, "freeze_bn": mode, "batch": B, "input": [H, W], **compare(alternate(fn, 1))}
                    print(f"{what} --freeze-bn {mode}: {entry['fused']['median_ms']:.2f} ms fused / "
                          f"{entry['torch']['median_ms']:.2f} ms torch (x {entry['ratio_torch_over_fused']:.3f})"
                          f"{'  FUSED SLOWER' if entry['fused_slower'] else ''}", flush=True)
                e2e.append(entry)
            del enc, disp_net, pose_net, opt, trainable, start, groups
            torch.cuda.empty_cache()

    result = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "site_repetitions_per_sample": args.inner,
              "hbm_bytes_per_s": HBM_BYTES_PER_S,
              "any_fused_slower": any(e.get("fused_slower", False) for e in sites + e2e), "sites": sites, "end_to_end": e2e}
    if os.path.exists(args.out):
        with open(args.out) as f:
            old = json.load(f)
        if "default_step_vs_parent" in old:
            result["default_step_vs_parent"] = old["default_step_vs_parent"]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps({k: v for k, v in result.items() if k not in ("sites", "end_to_end")}))


if __name__ == "__main__":
    main()
