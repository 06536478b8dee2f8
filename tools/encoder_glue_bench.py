"""The encoder's fused ops alone at one shape (default: the stem of configs[1], 12 x 64 x 128 x 416): wall time per op by
HIP events, and -- run under `rocprofv3 --kernel-trace --stats -d DIR -o trace -- python tools/encoder_glue_bench.py` --
per-kernel durations in DIR/trace_results.db, to set against the bytes each kernel moves."""
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
ident = torch.randn(args.shape, device=dev).requires_grad_()
g = torch.randn(args.shape, device=dev)
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


for name, ident_, relu, passes_f, passes_b in (("bn", None, False, 3, 5), ("bn_relu", None, True, 3, 5),
                                               ("bn_add_relu", ident, True, 4, 7)):
    y = E.bn_act(x, bn, ident_, relu=relu)
    tf = timed(lambda: E.bn_act(x, bn, ident_, relu=relu))
    tb = timed(lambda: torch.autograd.grad(y, [x] + ([ident_] if ident_ is not None else []), g, retain_graph=True))
    print(f"{name} {tuple(args.shape)}: forward {tf:.1f} us ({passes_f} x {mb:.1f} MB: {passes_f * mb / tf:.2f} TB/s)  "
          f"backward {tb:.1f} us ({passes_b} x {mb:.1f} MB: {passes_b * mb / tb:.2f} TB/s)")
xp = torch.relu(x.detach()).requires_grad_()
p = E.max_pool(xp)
gp = torch.randn_like(p)
tf = timed(lambda: E.max_pool(xp))
tb = timed(lambda: torch.autograd.grad(p, xp, gp, retain_graph=True))
print(f"max_pool {tuple(args.shape)}: forward {tf:.1f} us ({1.3125 * mb / tf:.2f} TB/s)  backward {tb:.1f} us "
      f"({1.3125 * mb / tb:.2f} TB/s)")
