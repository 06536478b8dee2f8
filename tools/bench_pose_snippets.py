"""Times scsfm_hip.snippets.evaluate_snippets on a KITTI-09-sized set (one sequence of 1,591 frames, 1,587 snippets of
five, float32 pair vectors, inputs resident on the device) against the numpy oracle's per-snippet loop on the host
(tests/pose_snippet_oracle.py: evaluate_sequence_loop, the reference's shape of the work) on the same data, and writes
both as JSON.  A host clock around the call, which ends in device-to-host copies (a synchronise); warmed up; medians.

    python tools/bench_pose_snippets.py profiles/pose_snippets_bench.json
"""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "sc-sfmlearner-release_amd")]

FRAMES, L, WARMUP, RUNS, ORACLE_RUNS = 1591, 5, 5, 30, 3


def main(path):
    import torch

    import odom_eval_oracle as O
    import pose_snippet_oracle as P
    from scsfm_hip import _lib
    from scsfm_hip.snippets import evaluate_snippets
    if not torch.cuda.is_available():
        raise SystemExit("this measurement needs a HIP device")
    rng = np.random.default_rng(9)
    v = rng.normal(0.0, 0.01, (FRAMES - 1, 6))
    v[:, 2] -= 0.4
    w = rng.normal(0.0, 0.01, (FRAMES - 1, 6))
    w[:, 2] -= 1.1
    vec32, gt = v.astype(np.float32), O.fold(O.euler_mat(w)).reshape(-1, 12)
    d_vec, d_gt = torch.from_numpy(vec32).cuda(), torch.from_numpy(gt).cuda()
    times = []
    for i in range(WARMUP + RUNS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = evaluate_snippets([d_vec], [d_gt], L)
        times.append(time.perf_counter() - t0)
    times = times[WARMUP:]
    mats = P.mats(vec32)
    oracle = []
    for _ in range(ORACLE_RUNS):
        t0 = time.perf_counter()
        want = P.evaluate_sequence_loop(mats, gt, L)
        oracle.append(time.perf_counter() - t0)
    rel = float(np.max(np.abs(res.errors[:, 0] - want["errors"][:, 0]) / np.abs(want["errors"][:, 0])))
    out = dict(what="evaluate_snippets, one sequence, inputs on the device, host clock around the call (ends in a "
                    "device-to-host copy); the numpy oracle's per-snippet loop on the host",
               device=torch.cuda.get_device_name(0), frames=FRAMES, snippets=len(res.errors), seq_length=L,
               vectors="float32", warmup=WARMUP, runs=RUNS,
               hip_ms_median=statistics.median(times) * 1e3, hip_ms_min=min(times) * 1e3, hip_ms_max=max(times) * 1e3,
               oracle_runs=ORACLE_RUNS, oracle_loop_ms_median=statistics.median(oracle) * 1e3,
               oracle_loop_ms_min=min(oracle) * 1e3, max_rel_ate_difference=rel,
               library_source_id=_lib.get_snip().source_id())
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "pose_snippets_bench.json"))
