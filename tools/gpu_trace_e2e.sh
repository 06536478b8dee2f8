#!/bin/bash
# rocprofv3 kernel trace of a few WHOLE training steps (nets + loss path + optimizer) -> e2e_kernels_<tag>.txt in the output directory:
# the project's own kernels and MIOpen's Winograd rows by launch size, over the whole trace and over the steps behind the
# warm-up alone, then the top kernels by total time.  The trace database goes to TRACE_DIR (default: a directory under
# /tmp), not into the output directory: only the summarised rows are kept.
#   bash tools/gpu_trace_e2e.sh [tag]
set -o pipefail
TAG=${1:-e2e}
export TMPDIR=/tmp
R=$PWD; O=$R/gpurun_out; mkdir -p $O
T=${TRACE_DIR:-/tmp/scsfm_trace_$TAG.$$}; mkdir -p $T
WARMUP=2; STEPS=5
cd /tmp
timeout -k 10 900 rocprofv3 --kernel-trace --stats -d $T -o trace -- python $R/bench.py --full --pmc-live 0 --steps $STEPS --warmup $WARMUP --loss-steps 2 --loss-warmup 1 --cpu-seconds 0 --graph 0 --kernel-iters 1 > $O/rocprof_$TAG.log 2>&1 \
  || { echo "the traced run failed"; tail -20 $O/rocprof_$TAG.log; exit 1; }
cd $R
python - $T/trace_results.db $WARMUP $STEPS <<'P' | tee $O/e2e_kernels_$TAG.txt
import sqlite3, sys
from collections import defaultdict
cur = sqlite3.connect(sys.argv[1]).cursor()
warmup, steps = int(sys.argv[2]), int(sys.argv[3])
n_steps = warmup + steps
cols = [d[0] for d in cur.execute("select * from kernels limit 1").description]
gx = next(c for c in ("grid_x", "grid_size_x", "grid_size") if c in cols)
wx = next(c for c in ("workgroup_x", "workgroup_size_x", "workgroup_size") if c in cols)
launches = cur.execute(f"select name, {gx}, {wx}, start, duration from kernels order by start").fetchall()
launches = [(" ".join(n.split()), g, w, s, d) for n, g, w, s, d in launches]
own = lambda n: "scsfm" in n or "miopenSp3AsmConv" in n  # noqa: E731

# the steps behind the warm-up: disp_head_fwd_kernel at its largest grid runs once per DispResNet pass, three times per
# step; from the first of step `warmup` to the first of the last step lie steps - 1 whole steps (a step's backward and
# optimizer, the next step's forward up to that kernel), with none of MIOpen's solver search
heads = [(g, s) for n, g, w, s, d in launches if "disp_head_fwd_kernel" in n]
big = max((g for g, s in heads), default=0)
marks = [s for g, s in heads if g == big]
steady = None
if len(marks) == 3 * n_steps:
    steady = (marks[3 * warmup], marks[3 * (n_steps - 1)])
    print(f"# steady = the {steps - 1} steps between the first full-resolution disp_head_fwd_kernel of step {warmup + 1} "
          f"and that of step {n_steps}; all = the whole trace / {n_steps} (the first step holds MIOpen's solver search)")
else:
    print(f"# {len(marks)} full-resolution disp_head_fwd_kernel launches, not {3 * n_steps}: no steady window; all = the "
          f"whole trace / {n_steps}")
rows = defaultdict(lambda: [0, 0.0, 0, 0.0])
for n, g, w, s, d in launches:
    if not own(n):
        continue
    r = rows[(n, g, w)]
    r[0] += 1
    r[1] += d / 1e3
    if steady and steady[0] <= s < steady[1]:
        r[2] += 1
        r[3] += d / 1e3
print("# steady: launches/step  us/step  avg_us | all: launches/step  us/step | grid_x x workgroup_x  kernel")
for (n, g, w), (c, t, cs, ts) in sorted(rows.items(), key=lambda kv: -kv[1][1]):
    k = steps - 1
    st = f"{cs / k:8.2f} {ts / k:10.1f} {ts / cs if cs else 0:8.1f}" if steady else " " * 28
    print(f"{st} | {c / n_steps:7.1f} {t / n_steps:10.1f} | {g:>12}x{w:<4} {n[:150]}")

if steady:  # MIOpen's Winograd launches share one grid: told apart by duration instead, in bins of 10 us
    print("#\n# steady: launches/step of the Winograd kernels by duration (us, bins of 10):")
    bins = defaultdict(int)
    for n, g, w, s, d in launches:
        if "miopenSp3AsmConv" in n and steady[0] <= s < steady[1]:
            bins[(n, int(d / 1e4) * 10)] += 1
    for n in sorted({n for n, b in bins}):
        row = "  ".join(f"{b}-{b + 10}: {c / (steps - 1):.2f}" for (m, b), c in sorted(bins.items()) if m == n)
        print(f"# {n}\n#   {row}")

if steady:  # the decoder's full-resolution backward as it ran: MIOpen picks its solvers anew in every process, so launch
    # counts of one of its kernels differ between two traces by more than a change does; the order of launches does not
    inside = [l for l in launches if steady[0] <= l[3] < steady[1]]
    first = [i for i, l in enumerate(inside) if "disp_head_bwd_kernel" in l[0] or "head_tail_bwd_kernel" in l[0]]
    if first:
        print("#\n# steady: the launches of the last DispResNet pass from the head's backward to level 1's ELU backward "
              "(duration us, grid_x x workgroup_x, kernel):")
        full = max(g for n, g, w, s, d in inside if "bias_elu_pad_fwd_kernel" in n) * 0.9
        for n, g, w, s, d in inside[first[-1]:first[-1] + 60]:
            print(f"# {d / 1e3:8.1f} {g:>12}x{w:<4} {n[:110]}")
            if "bias_elu_pad_bwd_kernel" in n and g < full:
                break

by_name = defaultdict(lambda: [0, 0.0])
for n, g, w, s, d in launches:
    by_name[n][0] += 1
    by_name[n][1] += d / 1e3
tot = sum(t for c, t in by_name.values())
print("#\n# the trace's largest kernels (launches, total, average, share of the trace):")
print(f"# {len(by_name)} distinct kernels, {len(launches)} launches, {tot / 1e3:.1f} ms of kernel time in the trace")
for n, (c, t) in sorted(by_name.items(), key=lambda kv: -kv[1][1])[:45]:
    print(f"{c:7d} {t:11.1f} us {t / c:9.1f} us {100 * t / tot:5.1f}%  {n[:150]}")
P
rc=$?
[ -n "$TRACE_DIR" ] || rm -rf $T
exit $rc
