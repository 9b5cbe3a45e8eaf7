"""Posterior motif-node profiles under the motif model: device time of elemdp_node_profile next to
elemdp_pair_posteriors and elemdp_context_profile of the same process, from the engine's HIP events (last_timing: ms[0] the whole
call with the copy of the result, ms[1] the sum passes + the call's own kernels).  Prints one JSON line per shape.

    python tools/node_bench.py [n] [L ...]       (default: 10000 sequences of L = 200 and of L = 300, pattern ((.*.)))

The node kernel's share of the call comes from a separate `rocprofv3 --kernel-trace --stats` run of this script: k_node_pos
against the sum passes (k4_in / k4_in_ext / k4_out_ext / k4_r7 / k4_out / k5_pick)."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from rnaelem_amd import api, synth  # noqa: E402


def timed(call, eng):
    reps = []
    for _ in range(3):
        t0 = time.time()
        res = call()
        wall = time.time() - t0
        reps.append((eng.last_timing().tolist(), wall))
    return res, min(reps, key=lambda r: r[0][0]), [r[0][0] for r in reps]


def main():
    args = sys.argv[1:]
    n = int(args[0]) if args else 10000
    lengths = [int(v) for v in args[1:]] or [200, 300]
    pattern = os.environ.get("NODE_BENCH_PATTERN", "((.*.))")
    for L in lengths:
        eng = api.Engine(pattern, "~T2004~", 50, 30, 1e-4, 0.1, 0, 0)
        seqs, quals = synth.synth_batch(n, L, seed=L)
        eng.load_batch(seqs, quals)
        x = eng.initial_params(1.0)
        x[:-2] += 0.1
        eng.scan(x)                           # (warm-up: code objects, table slots)
        eng.pair_posteriors(x, 1e-3)
        _, pbest, pall = timed(lambda: eng.pair_posteriors(x, 1e-3), eng)
        eng.context_profiles(x)
        _, cbest, call_ = timed(lambda: eng.context_profiles(x), eng)
        eng.node_profiles(x)
        prof, best, all_ms = timed(lambda: eng.node_profiles(x), eng)
        mean = sum(p.sum(axis=0) for p in prof) / sum(len(p) for p in prof)
        names = eng.describe()["node"]
        print(json.dumps(dict(pattern=pattern, n=n, L=L, call_ms=best[0][0], sums_and_node_kernel_ms=best[0][1],
                              log_space_sequences=best[0][2], call_ms_all=all_ms, host_wall_s=round(best[1], 3),
                              pair_call_ms=pbest[0][0], pair_sums_and_kernels_ms=pbest[0][1], pair_call_ms_all=pall,
                              context_call_ms=cbest[0][0], context_sums_and_kernels_ms=cbest[0][1], context_call_ms_all=call_,
                              node_kernel_over_pair_sums=round((best[0][1] - pbest[0][1]) / pbest[0][1], 4),
                              mean_profile={"%d%s" % (k, c): round(float(v), 5) for k, (c, v) in enumerate(zip(names, mean))})),
              flush=True)


if __name__ == "__main__":
    main()
