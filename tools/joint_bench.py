"""Joint node-by-context posteriors under the motif model: device time of elemdp_joint_profile next to
elemdp_pair_posteriors, elemdp_context_profile and elemdp_node_profile of the same process, one after the other on the same batch,
from the engine's HIP events (last_timing: ms[0] the whole call with the copy of its result, ms[1] the sum passes + the call's own
kernels); best of three.  The call replaces a context call plus a node call, so their sum is the yardstick.  Prints one JSON line
per shape.

    python tools/joint_bench.py [n] [L ...]       (default: 10000 sequences of L = 200 and of L = 300, pattern ((.*.)))

The share of each kernel comes from a separate `rocprofv3 --kernel-trace --stats` run of this script: k_joint_rows, k_joint_pos and
k_joint_counts against the sum passes (k4_in / k4_in_ext / k4_out_ext / k4_r7 / k4_out / k5_pick)."""
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
    pattern = os.environ.get("JOINT_BENCH_PATTERN", "((.*.))")
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
        _, nbest, nall = timed(lambda: eng.node_profiles(x), eng)
        eng.joint_profiles(x)
        counts, best, all_ms = timed(lambda: eng.joint_profiles(x), eng)
        _, fbest, fall = timed(lambda: eng.joint_profiles(x, profile=True), eng)
        logo = api.motif_logo(counts)
        names = eng.describe()["node"]
        yard0, yard1 = cbest[0][0] + nbest[0][0], cbest[0][1] + nbest[0][1]
        print(json.dumps(dict(pattern=pattern, n=n, L=L, call_ms=best[0][0], sums_and_joint_kernels_ms=best[0][1],
                              log_space_sequences=best[0][2], call_ms_all=all_ms, host_wall_s=round(best[1], 3),
                              call_with_profile_ms=fbest[0][0], call_with_profile_ms_all=fall,
                              pair_call_ms=pbest[0][0], pair_sums_and_kernels_ms=pbest[0][1], pair_call_ms_all=pall,
                              context_call_ms=cbest[0][0], context_sums_and_kernels_ms=cbest[0][1], context_call_ms_all=call_,
                              node_call_ms=nbest[0][0], node_sums_and_kernels_ms=nbest[0][1], node_call_ms_all=nall,
                              yardstick_context_plus_node_ms=yard0, call_over_yardstick=round(best[0][0] / yard0, 4),
                              kernels_over_yardstick=round(best[0][1] / yard1, 4),
                              joint_kernels_over_pair_sums=round((best[0][1] - pbest[0][1]) / pbest[0][1], 4),
                              occurrences={"%d%s" % (k, c): round(float(v), 2) for k, (c, v) in enumerate(zip(names, logo["occurrences"]))},
                              information={"%d%s" % (k, c): round(float(v), 4) for k, (c, v) in enumerate(zip(names, logo["information"]))})),
              flush=True)


if __name__ == "__main__":
    main()
