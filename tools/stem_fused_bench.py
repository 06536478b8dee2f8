"""The fused stem (bn_act(..., pool=True)) alone at one shape (default: the stem of configs[1], 12 x 64 x 128 x 416)
beside the unfused pair it replaces: wall time per op by HIP events, and -- run under `rocprofv3 --kernel-trace --stats -d
DIR -o trace -- python tools/stem_fused_bench.py` -- per-kernel durations in DIR/trace_results.db, to set against the
bytes each kernel moves (in units of T, the stem tensor: statistics 1, forward 2.31, each backward launch 1.31 without
and 2.31 with a gradient on f0, plus 1 for the dx it writes)."""
import argparse
import os
import sys

import torch
import torch.nn as nn

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "sc-sfmlearner-release_amd"))
from scsfm_hip import encoder as E  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--shape", type=int, nargs=4, default=[12, 64, 128, 416])
ap.add_argument("--iters", type=int, default=20)
args = ap.parse_args()
dev = "cuda"
x = torch.randn(args.shape, device=dev).requires_grad_()
bn = nn.BatchNorm2d(args.shape[1]).to(dev).train()
mb = x.numel() * 4 / 1e6


def timed(fn):
    for _ in range(3):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(args.iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / args.iters


f0, pooled = E.bn_act(x, bn, pool=True)
g0, gp = torch.randn_like(f0), torch.randn_like(pooled)
tf = timed(lambda: E.bn_act(x, bn, pool=True))
tb = timed(lambda: torch.autograd.grad([pooled], [x], [gp], retain_graph=True))
tbs = timed(lambda: torch.autograd.grad([pooled, f0], [x], [gp, g0], retain_graph=True))
print(f"fused stem {tuple(args.shape)}: forward {tf:.1f} us (3.31 x {mb:.1f} MB: {3.31 * mb / tf:.2f} TB/s)  backward "
      f"{tb:.1f} us (3.62 T: {3.62 * mb / tb:.2f} TB/s)  backward with a gradient on f0 {tbs:.1f} us (5.62 T: "
      f"{5.62 * mb / tbs:.2f} TB/s)")
y = E.bn_act(x, bn)
p = E.max_pool(y)
tf = timed(lambda: E.max_pool(E.bn_act(x, bn)))
tb = timed(lambda: torch.autograd.grad([p], [x], [gp], retain_graph=True))
tbs = timed(lambda: torch.autograd.grad([p, y], [x], [gp, g0], retain_graph=True))
print(f"unfused pair {tuple(args.shape)}: forward {tf:.1f} us (4.31 T)  backward {tb:.1f} us (6.31 T)  backward with a "
      f"gradient on f0 {tbs:.1f} us (9.31 T)")
