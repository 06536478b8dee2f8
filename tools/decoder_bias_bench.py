"""The decoder-bias kernels (libscsfm_decb.so) alone, next to the libscsfm_nets.so kernels they replace, at the level-0
and level-1 shapes of configs[1] (batch 12, 256 x 832).

    rocprofv3 --kernel-trace -d <dir> -o trace -- python tools/decoder_bias_bench.py --iters 20
    python tools/decoder_bias_bench.py --report <dir>/trace_results.db

The first form only launches: every kernel `--iters` times after 3 warm-up calls, one shape after the other.  The second
reads the trace and prints, per kernel and shape (matched by kernel name and launch size), the median duration, the
bytes the call has to move (inputs read once, outputs written once; the backward of up_cat_pad reads the saved output
only on the even rows of its first Ca planes, counted as half of them) over that duration, and its share of the
6.29 TB/s copy rate.  The backwards run with and without the bias sum, whose second launch (bias_sum_kernel) is listed
beside them."""
import argparse
import os
import sqlite3
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sc-sfmlearner-release_amd"))

COPY_RATE = 6.29e12  # bytes/s, the measured copy rate of one MI355X
B = 12
# level: (elu_pad's [C, H, W], up_cat_pad's [Ca, Cs, H, W], the head's [H, W])
LEVELS = {0: ((16, 256, 832), (16, 0, 128, 416), (256, 832)),
          1: ((32, 128, 416), (32, 64, 64, 208), (128, 416))}


def _grid(nseg):
    return -(-nseg // 4) * 256


def _chunks(n):
    return -(-n // 256)


def cases():
    """-> [(label, kernel-name fragment, work-items of the launch, bytes moved)]"""
    out = []
    for lvl, ((C, H, W), (Ca, Cs, h, w), (hh, hw)) in LEVELS.items():
        n, npad = B * C * H * W, B * C * (H + 2) * (W + 2)
        fwd, bwd = _grid(B * C * (H + 2) * _chunks(W + 2)), _grid(B * C * H * _chunks(W))
        ws = 8 * B * C * H * _chunks(W)
        out += [(f"L{lvl} elu_pad fwd", "scsfm_nets::pad_fwd_kernel<true>", fwd, 4 * (n + npad)),
                (f"L{lvl} bias_elu_pad fwd", "scsfm_decb::bias_elu_pad_fwd_kernel", fwd, 4 * (n + npad)),
                (f"L{lvl} elu_pad bwd", "scsfm_nets::pad_bwd_kernel<true>", bwd, 4 * (npad + 2 * n)),
                (f"L{lvl} bias_elu_pad bwd, no sum", "scsfm_decb::bias_elu_pad_bwd_kernel<false>", bwd, 4 * (npad + 2 * n)),
                (f"L{lvl} bias_elu_pad bwd, sum", "scsfm_decb::bias_elu_pad_bwd_kernel<true>", bwd,
                 4 * (npad + 2 * n) + ws),
                (f"L{lvl} bias_elu_pad sum of {ws // 8} partials", "scsfm_decb::bias_sum_kernel", C * 256, ws)]
        na, ns = B * Ca * h * w, B * Cs * 4 * h * w
        npad = B * (Ca + Cs) * (2 * h + 2) * (2 * w + 2)
        npad_a = B * Ca * (2 * h + 2) * (2 * w + 2)
        fwd = _grid(B * (Ca + Cs) * (2 * h + 2) * _chunks(2 * w + 2))
        bwd = _grid(B * Ca * h * _chunks(w) + B * Cs * 2 * h * _chunks(2 * w))
        ws = 8 * B * Ca * h * _chunks(w)
        moved_b = 4 * (npad + npad_a // 2 + na + ns)
        out += [(f"L{lvl} up_cat_pad fwd", "scsfm_nets::up_cat_pad_fwd_kernel", fwd, 4 * (na + ns + npad)),
                (f"L{lvl} bias_up_cat_pad fwd", "scsfm_decb::bias_up_cat_pad_fwd_kernel", fwd, 4 * (na + ns + npad)),
                (f"L{lvl} up_cat_pad bwd", "scsfm_nets::up_cat_pad_bwd_kernel", bwd, moved_b),
                (f"L{lvl} bias_up_cat_pad bwd, no sum", "scsfm_decb::bias_up_cat_pad_bwd_kernel<false>", bwd, moved_b),
                (f"L{lvl} bias_up_cat_pad bwd, sum", "scsfm_decb::bias_up_cat_pad_bwd_kernel<true>", bwd, moved_b + ws),
                (f"L{lvl} bias_up_cat_pad sum of {ws // 8} partials", "scsfm_decb::bias_sum_kernel", Ca * 256, ws)]
        n = B * hh * hw
        g = _grid(B * _chunks(hh * hw))
        ws = 8 * B * _chunks(hh * hw)
        out += [(f"L{lvl} disp_head fwd", "scsfm_decb::disp_head_fwd_kernel", g, 4 * 3 * n),
                (f"L{lvl} disp_head bwd, no sum", "scsfm_decb::disp_head_bwd_kernel<false>", g, 4 * 3 * n),
                (f"L{lvl} disp_head bwd, sum", "scsfm_decb::disp_head_bwd_kernel<true>", g, 4 * 3 * n + ws),
                (f"L{lvl} disp_head sum of {ws // 8} partials", "scsfm_decb::bias_sum_kernel", 256, ws)]
    return out


def run(iters):
    import torch
    from scsfm_hip import decoder as D, decoder_bias as DB
    dev = "cuda"
    for lvl, ((C, H, W), (Ca, Cs, h, w), (hh, hw)) in LEVELS.items():
        def rnd(*shape):
            return torch.randn(*shape, device=dev)

        def both(fwd, inputs, bias):
            """forward and backward `iters` + 3 times: with the bias's gradient, then with the bias frozen"""
            for frozen in (False, True):
                bias.requires_grad_(not frozen)
                for _ in range(iters + 3):
                    out = fwd()
                    torch.autograd.grad(out, inputs + ([] if frozen or bias is None else [bias]), gp_like(out))
            torch.cuda.synchronize()

        cache = {}

        def gp_like(out):
            if out.shape not in cache:
                cache.clear()
                cache[out.shape] = torch.randn_like(out)
            return cache[out.shape]

        x, bias = rnd(B, C, H, W).requires_grad_(), rnd(C)
        both(lambda: DB.elu_pad(x, bias), [x], bias)
        for _ in range(iters + 3):
            out = D.elu_pad(x)
            torch.autograd.grad(out, [x], gp_like(out))
        a, bias = rnd(B, Ca, h, w).requires_grad_(), rnd(Ca)
        skip = rnd(B, Cs, 2 * h, 2 * w).requires_grad_() if Cs else None
        ins = [a] + ([skip] if Cs else [])
        both(lambda: DB.up_cat_pad(a, bias, skip), ins, bias)
        for _ in range(iters + 3):
            out = D.up_cat_pad(a, skip)
            torch.autograd.grad(out, ins, gp_like(out))
        x, bias = rnd(B, 1, hh, hw).requires_grad_(), rnd(1)
        both(lambda: DB.disp_head(x, bias, 10, 0.01), [x], bias)
        del x, a, skip, out
        cache.clear()
        torch.cuda.empty_cache()
    print(f"launched every kernel {iters} + 3 times at levels {sorted(LEVELS)}")


def report(db):
    cur = sqlite3.connect(db).cursor()
    cols = [d[0] for d in cur.execute("select * from kernels limit 1").description]
    gx = next(c for c in ("grid_x", "grid_size_x", "grid_size") if c in cols)
    rows = cur.execute(f"select name, {gx}, duration from kernels").fetchall()
    print(f"# copy rate {COPY_RATE / 1e12:.2f} TB/s; durations are medians over the launches of a kernel at one launch size")
    print("# launches  median_us   MB moved   TB/s  of copy rate  kernel at shape")
    for label, frag, grid, moved in cases():
        ds = sorted(d for name, g, d in rows if frag in " ".join(name.split()) and g == grid)
        if not ds:
            print(f"#       0          -  {moved / 1e6:9.1f}      -        -      {label}  ({frag}, {grid} work-items: not in the trace)")
            continue
        med = ds[len(ds) // 2] / 1e3
        rate = moved / (med * 1e-6)
        print(f"{len(ds):9d} {med:10.1f}  {moved / 1e6:9.1f} {rate / 1e12:6.2f} {100 * rate / COPY_RATE:8.1f} %     {label}")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--report", metavar="DB", help="read a rocprofv3 trace (trace_results.db) instead of launching")
    args = ap.parse_args()
    report(args.report) if args.report else run(args.iters)
