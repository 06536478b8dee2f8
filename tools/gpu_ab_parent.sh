#!/bin/bash
# A/B of the headline against another checkout of this repository (usually the parent commit), in one GPU session:
#   bash tools/gpu_ab_parent.sh <built checkout of the other tree> <output directory> [runs=3]
# Plain `bench.py --gpus 1 --steps 50 --warmup 10` alternating between this tree and the other one (ms_per_step of each
# run), then `bench.py --dump-outputs` (3 steps, 2 warm-up) of this tree, the other tree and the other tree again,
# compared file by file.  Both trees must have been built beforehand (python __graft_entry__.py).  Every GPU step runs
# under its own time limit and the first failure ends the script.  Output: ab.txt and dumps.txt in the output directory.
set -o pipefail
export TMPDIR=/tmp
R=$PWD; P=$(cd "$1" && pwd) || exit 2; [ -n "$2" ] || exit 2; mkdir -p "$2"; O=$(cd "$2" && pwd); N=${3:-3}
: > $O/ab.txt
for i in $(seq $N); do
  for side in pr parent; do
    D=$R; [ $side = parent ] && D=$P
    (cd $D && timeout -k 10 300 python bench.py --gpus 1 --steps 50 --warmup 10 2>$O/bench_${side}_$i.err | tail -1 > $O/bench_${side}_$i.json) \
      || { echo "bench $side $i failed"; tail -5 $O/bench_${side}_$i.err; exit 1; }
    python -c "import json,sys; print(sys.argv[2], sys.argv[3], json.load(open(sys.argv[1]))['ms_per_step'])" \
      $O/bench_${side}_$i.json $side $i | tee -a $O/ab.txt
  done
done
for tag in pr parent parent2; do
  D=$R; [ $tag = pr ] || D=$P
  (cd $D && timeout -k 10 300 python bench.py --gpus 1 --steps 3 --warmup 2 --dump-outputs $O/dump_$tag > $O/dump_$tag.log 2>&1) \
    || { echo "dump $tag failed"; tail -5 $O/dump_$tag.log; exit 1; }
done
python - $O/dump_pr $O/dump_parent $O/dump_parent2 <<'P' | tee $O/dumps.txt
import glob, os, sys
import numpy as np
pr, parent, parent2 = sys.argv[1:4]
for f in sorted(glob.glob(os.path.join(pr, "*.npy"))):
    n = os.path.basename(f)
    a, b, c = (np.load(os.path.join(d, n)).astype(np.float64) for d in (pr, parent, parent2))
    print(f"{n}: pr==parent bitwise {np.array_equal(a, b)}  max|pr-parent| {np.abs(a - b).max():.3e}  "
          f"max|parent-parent2| {np.abs(b - c).max():.3e}  scale {np.abs(b).max():.3e}")
P
