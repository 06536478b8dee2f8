"""Every distinct convolution problem of DispResNet(18) and PoseResNet(18) at configs[1] (batch 12, 256 x 832, fp32, the
fused paths), alone: which kernels MIOpen launches for its weight gradient, its data gradient and its forward, how long
they take, and what the shape allows.

    rocprofv3 --kernel-trace -d <dir> -o trace -- python tools/conv_layers_bench.py --iters 10 --out <dir>/segments.json
    python tools/conv_layers_bench.py --report <dir>/trace_results.db --segments <dir>/segments.json

The first form collects the problems (a dispatch mode records every aten.convolution of one training-mode forward of
each net, with the module that owns the weight) and launches, per problem, aten.convolution_backward with the output mask
[False, True, False] (weight only), with [True, False, False] (input only) and the forward, `--iters` times each after 3
warm-up calls; for the problems scsfm_hip.conv_wrw covers it also launches libscsfm_wrw.so's weight gradient (`wrw_hip`)
and libscsfm_dgrad.so's data gradient (`bwd_hip`).  Each
timed stretch lies between two marker kernels (erfinv in front, digamma behind: nothing else here launches them), so
the report can tell which kernels belong to it.  The second form reads the trace and prints one row per problem and
direction: launches per step of the training loop (3 DispResNet passes, 4 PoseResNet passes), the kernels of one call
(convolution, transposes, casts, zero-fill) with their launches per call and median durations, their sum, the FLOPs
and the bytes the operands hold, and the two floors: FLOPs / 157 TFLOP/s (the fp32 matrix peak) and bytes / 6.29 TB/s
(the measured copy rate).

Behind the convolution problems comes the backward of the decoder's full-resolution tail (level 0: ELU, pad, disparity
head), as the launches it used to be (direction `tail`: the head's sigmoid backward with its bias sum, MIOpen's data
gradient of the 16 -> 1 convolution, the pad / ELU backward with its bias sum) and as libscsfm_dgrad.so's one pass
(`tail_hip`); its bytes are what the one pass has to move (the padded tensor, the gradient it stores, three planes).
`--tail-only` launches these two stretches alone, `--dgrad-only` these and the data gradients (`bwd`, `bwd_hip`) of the
problems libscsfm_dgrad.so covers.

`--pw-only` launches, for the 1x1 convolutions scsfm_hip.conv1x1 covers (the encoders' down-sample branches and the pose
decoder's squeeze) and nothing else, MIOpen's weight gradient beside libscsfm_pw.so's two launches (`wrw`, `wrw_hip`) and,
for stride 2, MIOpen's data gradient beside the library's one (`bwd`, `bwd_hip`).  The report's last column is the rate
at which a call moves its operands' bytes, against the copy rate."""
import argparse
import json
import os
import re
import sqlite3
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sc-sfmlearner-release_amd"))
sys.path.insert(0, ROOT)

COPY_RATE = 6.29e12    # bytes/s, the measured copy rate of one MI355X
MATRIX_PEAK = 157.3e12  # fp32 FLOP/s of v_mfma_f32_*_f32
B, H, W = 12, 256, 832
PASSES = {"disp": 3, "pose": 4}  # per training step with two reference frames
DIRECTIONS = ("wrw", "bwd", "fwd", "wrw_hip", "bwd_hip", "tail", "tail_hip")
TAIL_C = 16


def collect():
    """-> [problem dict] of both nets: distinct (x shape, w shape, stride, padding, dilation, groups), with the names of
    the modules that own the weights and the calls per pass"""
    import torch
    from torch.utils._python_dispatch import TorchDispatchMode

    import models

    class Recorder(TorchDispatchMode):
        def __init__(self, owner):
            super().__init__()
            self.owner, self.calls = owner, []

        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            if func is torch.ops.aten.convolution.default:
                x, w, bias, stride, padding, dilation, transposed, _, groups = args[:9]
                assert not transposed
                self.calls.append((tuple(x.shape), tuple(w.shape), tuple(stride), tuple(padding), tuple(dilation),
                                   int(groups), self.owner.get(w.data_ptr(), "?")))
            return func(*args, **(kwargs or {}))

    torch.manual_seed(0)
    problems = {}
    for net_name, make, inputs in (("disp", lambda: models.DispResNet(18, False), 1),
                                   ("pose", lambda: models.PoseResNet(18, False), 2)):
        net = make().cuda().train()
        owner = {m.weight.data_ptr(): name for name, m in net.named_modules() if isinstance(m, torch.nn.Conv2d)}
        imgs = [torch.randn(B, 3, H, W, device="cuda") for _ in range(inputs)]
        with Recorder(owner) as rec:
            net(*imgs)
        for xs, ws, st, pd, dl, gr, name in rec.calls:
            key = (xs, ws, st, pd, dl, gr)
            p = problems.setdefault(key, {"x": xs, "w": ws, "stride": st, "padding": pd, "dilation": dl, "groups": gr,
                                          "layers": [], "per_step": 0})
            p["layers"].append(f"{net_name}.{name}")
            p["per_step"] += PASSES[net_name]
        del net, imgs
        torch.cuda.empty_cache()
    return list(problems.values())


def out_shape(p):
    (b, _, h, w), (co, _, kh, kw) = p["x"], p["w"]
    ho = (h + 2 * p["padding"][0] - p["dilation"][0] * (kh - 1) - 1) // p["stride"][0] + 1
    wo = (w + 2 * p["padding"][1] - p["dilation"][1] * (kw - 1) - 1) // p["stride"][1] + 1
    return (b, co, ho, wo)


def tail_calls(torch):
    """-> the tail's problem entry and its two calls"""
    from scsfm_hip import _lib, decoder_dgrad as DG
    from scsfm_hip.decoder_bias import _bias_sum_buffers
    q = torch.rand(B, TAIL_C, H + 2, W + 2, device="cuda") * 3 - 1
    y = torch.rand(B, 1, H, W, device="cuda")
    g_out = torch.randn(B, 1, H, W, device="cuda")
    w = torch.randn(1, TAIL_C, 3, 3, device="cuda")
    decb = _lib.get_decb()
    stream = torch.cuda.current_stream().cuda_stream

    def parts():
        g = torch.empty_like(y)
        ws, g_bias = _bias_sum_buffers(decb, y, True, B, 1, 1, H * W)
        decb.call("scsfm_decb_disp_head_bwd_f32", B, 1, H, W, 10.0, g_out.data_ptr(), y.data_ptr(), g.data_ptr(),
                  ws.data_ptr(), g_bias.data_ptr(), stream)
        gq = torch.ops.aten.convolution_backward(g, q, w, None, [1, 1], [0, 0], [1, 1], False, [0, 0], 1,
                                                 [True, False, False])[0]
        g_b = torch.empty(B, TAIL_C, H, W, device="cuda")
        ws, g_bias = _bias_sum_buffers(decb, y, True, B, TAIL_C, H, W)
        decb.call("scsfm_decb_bias_elu_pad_bwd_f32", B, TAIL_C, H, W, gq.data_ptr(), q.data_ptr(), g_b.data_ptr(),
                  ws.data_ptr(), g_bias.data_ptr(), stream)
        return g_b

    problem = {"x": tuple(q.shape), "w": tuple(w.shape), "stride": (1, 1), "padding": (0, 0), "dilation": (1, 1),
               "groups": 1, "layers": ["disp.decoder: the tail of level 0, backward"], "per_step": PASSES["disp"]}
    return problem, {"tail": parts, "tail_hip": lambda: DG.tail_bwd(q, y, g_out, w, 10.0)}


def run(iters, out, tail_only=False, dgrad_only=False, pw_only=False):
    import torch

    from bench import MIOPEN_SOLVERS_NEVER_CHOSEN
    for k in MIOPEN_SOLVERS_NEVER_CHOSEN:  # (the search space of bench.py's runs)
        os.environ.setdefault(k, "0")
    from scsfm_hip import conv_wrw as CW, conv1x1 as PW
    problems = [] if tail_only else collect()
    pointwise = lambda p: (p["w"][2:] == (1, 1) and p["padding"] == (0, 0) and p["dilation"] == (1, 1)  # noqa: E731
                           and p["groups"] == 1 and p["stride"][0] == p["stride"][1]
                           and PW.covers(p["w"][1], p["w"][0], p["stride"][0]))
    if pw_only:
        problems = [p for p in problems if pointwise(p)]
    covered = lambda p: (p["w"][2:] == (3, 3) and p["stride"] == (1, 1) and p["padding"] == (0, 0)  # noqa: E731
                         and p["groups"] == 1 and CW.dgrad_covers(p["w"][1], p["w"][0]))
    if dgrad_only:
        problems = [p for p in problems if covered(p)]
    marker = torch.rand(64, device="cuda") * 0.5
    segments = []

    def stretch(pi, d, call):
        for _ in range(3):
            call()
        torch.cuda.synchronize()
        torch.erfinv(marker)
        for _ in range(iters):
            call()
        torch.digamma(marker)
        torch.cuda.synchronize()
        segments.append({"problem": pi, "direction": d, "iters": iters})

    for pi, p in enumerate(problems):
        x = torch.randn(*p["x"], device="cuda")
        w = torch.randn(*p["w"], device="cuda")
        gy = torch.randn(*out_shape(p), device="cuda")
        conv = (list(p["stride"]), list(p["padding"]), list(p["dilation"]), False, [0, 0], p["groups"])

        def backward(mask):
            return torch.ops.aten.convolution_backward(gy, x, w, None, *conv, mask)

        calls = {"wrw": lambda: backward([False, True, False]), "bwd": lambda: backward([True, False, False]),
                 "fwd": lambda: torch.ops.aten.convolution(x, w, None, *conv)}
        plain3x3 = p["w"][2:] == (3, 3) and p["stride"] == (1, 1) and p["padding"] == (0, 0) and p["groups"] == 1
        if plain3x3 and CW.covers(p["w"][1], p["w"][0]):
            calls["wrw_hip"] = lambda: CW.weight_grad(x, gy)
        if covered(p):
            calls["bwd_hip"] = lambda: CW.data_grad(gy, w)
        if pointwise(p):
            s = p["stride"][0]
            calls["wrw_hip"] = lambda: PW.weight_grad(x, gy, s)
            if PW.dgrad_covers(p["w"][1], p["w"][0], s):
                calls["bwd_hip"] = lambda: PW.data_grad(gy, w, p["x"][2], p["x"][3])
        if dgrad_only:
            calls = {d: c for d, c in calls.items() if d in ("bwd", "bwd_hip")}
        if pw_only:
            calls = {d: c for d, c in calls.items() if d != "fwd" and (d != "bwd" or "bwd_hip" in calls)}
        for d in DIRECTIONS:
            if d in calls:
                stretch(pi, d, calls[d])
        del x, w, gy
        torch.cuda.empty_cache()
    if not pw_only:
        tail, calls = tail_calls(torch)
        problems.append(tail)
        for d, call in calls.items():
            stretch(len(problems) - 1, d, call)
    with open(out, "w") as f:
        json.dump({"problems": problems, "segments": segments}, f, indent=1)
    print(f"launched {len(segments)} stretches of {iters} calls over {len(problems)} problems; wrote {out}")


def short(name):
    name = " ".join(name.split())
    name = re.sub(r"^void ", "", name)
    m = re.match(r"([\w:]+)", name)
    return (m.group(1) if m else name)[:60]


def report(db, seg_file):
    meta = json.load(open(seg_file))
    problems, segments = meta["problems"], meta["segments"]
    cur = sqlite3.connect(db).cursor()
    cols = [d[0] for d in cur.execute("select * from kernels limit 1").description]
    start = next(c for c in ("start", "start_timestamp", "start_time", "begin") if c in cols)
    rows = cur.execute(f"select name, {start}, duration from kernels order by {start}").fetchall()
    stretches, inside = [], None
    for name, _, dur in rows:
        if "erfinv" in name:
            inside = []
        elif "digamma" in name:
            if inside is not None:
                stretches.append(inside)
            inside = None
        elif inside is not None:
            inside.append((short(name), dur / 1e3))
    assert len(stretches) == len(segments), (len(stretches), len(segments))
    print(f"# configs[1]: batch {B}, {H} x {W}, fp32.  floors: FLOPs / {MATRIX_PEAK / 1e12:.1f} TFLOP/s, operand "
          f"bytes / {COPY_RATE / 1e12:.2f} TB/s.")
    print("# per row: launches/step of this problem, direction, sum of the medians of one call's kernels, spread of "
          "the calls' totals (max - min), GFLOP, MB, matrix floor, byte floor, sum / larger floor; then the kernels")
    print("# (launches per call x median us)")
    for seg, ks in zip(segments, stretches):
        p = problems[seg["problem"]]
        n = seg["iters"]
        xs, ws, ys = p["x"], p["w"], out_shape(p)
        numel = lambda s: s[0] * s[1] * s[2] * s[3]  # noqa: E731
        flop = 2.0 * numel(ys) * ws[1] * ws[2] * ws[3]
        moved = 4.0 * {"wrw": numel(xs) + numel(ys), "wrw_hip": numel(xs) + numel(ys), "bwd": numel(ys) + numel(xs),
                       "bwd_hip": numel(ys) + numel(xs),
                       "fwd": numel(xs) + numel(ys), "tail": numel(xs) + (ws[1] + 3) * numel(ys),
                       "tail_hip": numel(xs) + (ws[1] + 3) * numel(ys)}[seg["direction"]] + 4.0 * numel(ws)
        by_name = {}
        for name, dur in ks:
            by_name.setdefault(name, []).append(dur)
        total, parts = 0.0, []
        for name, ds in by_name.items():
            ds.sort()
            med, per_call = ds[len(ds) // 2], len(ds) / n
            total += med * per_call
            parts.append(f"{name} {per_call:g} x {med:.1f}")
        # the calls' own totals: the trace is in launch order and every call launches the same sequence
        per = len(ks) // n if n and len(ks) % n == 0 else 0
        sums = sorted(sum(d for _, d in ks[i * per:(i + 1) * per]) for i in range(n)) if per else []
        spread = f"{sums[-1] - sums[0]:6.1f}" if sums else "     ?"
        f_mat, f_byte = flop / MATRIX_PEAK * 1e6, moved / COPY_RATE * 1e6
        layers = p["layers"]
        label = layers[0] + (f" (+{len(layers) - 1})" if len(layers) > 1 else "")
        print(f"{p['per_step']:3d} {seg['direction']:8s} {total:8.1f} us  spread {spread}  {flop / 1e9:6.2f} GFLOP "
              f"{moved / 1e6:7.1f} MB  floors {f_mat:6.1f} {f_byte:6.1f} us  x{total / max(f_mat, f_byte):5.2f}  "
              f"{ws[1]}->{ws[0]} {ws[2]}x{ws[3]} s{p['stride'][0]} p{p['padding'][0]} @ {ys[2]}x{ys[3]}  {label}  "
              f"{moved / total / 1e3:5.0f} GB/s = {100 * moved / total / 1e3 / (COPY_RATE / 1e9):3.0f}% of the copy rate")
        print("        " + "; ".join(parts))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default="segments.json", help="where the launching form writes its list of stretches")
    ap.add_argument("--report", metavar="DB", help="read a rocprofv3 trace (trace_results.db) instead of launching")
    ap.add_argument("--segments", default="segments.json", help="the launching form's --out, for --report")
    ap.add_argument("--tail-only", action="store_true", help="launch the two stretches of the decoder's tail alone")
    ap.add_argument("--dgrad-only", action="store_true",
                    help="launch the tail and the data gradients of the problems libscsfm_dgrad.so covers alone")
    ap.add_argument("--pw-only", action="store_true",
                    help="launch the weight and data gradients of the 1x1 convolutions libscsfm_pw.so covers alone")
    args = ap.parse_args()
    report(args.report, args.segments) if args.report else run(args.iters, args.out, args.tail_only, args.dgrad_only,
                                                               args.pw_only)
