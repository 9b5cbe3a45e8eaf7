"""Accessibility under the motif model: device time of elemdp_accessibility next to elemdp_pair_posteriors
and elemdp_context_profile of the same process -- all three run one sum pass --, from the engine's HIP events (last_timing: ms[0]
the whole call including the copy to the host, ms[1] sum passes + the call's kernels), best of three.  Prints one JSON line per
shape.

    python tools/access_bench.py [n] [L ...]       (default: 10000 sequences of L = 200 and of L = 300, pattern ((.*.)), U = 16)

The per-kernel split comes from a separate `rocprofv3 --kernel-trace --stats` run of this script: k_access_chains and k_access_seq
against the sum passes (k4_in / k4_in_ext / k4_out_ext / k4_r7 / k4_out) and the kernels of the other two calls."""
import json
import os
import sys
import time

import numpy as np

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
    pattern = os.environ.get("ACCESS_BENCH_PATTERN", "((.*.))")
    width = int(os.environ.get("ACCESS_BENCH_WIDTH", "16"))
    for L in lengths:
        eng = api.Engine(pattern, "~T2004~", 50, 30, 1e-4, 0.1, 0, 0)
        if os.environ.get("ACCESS_BENCH_TERMS"):       # (bits: 1 loop runs, 2 exterior, 4 tails behind a branch, 8 leading bases)
            eng.set_option("access_terms", int(os.environ["ACCESS_BENCH_TERMS"]))
        seqs, quals = synth.synth_batch(n, L, seed=L)
        eng.load_batch(seqs, quals)
        x = eng.initial_params(1.0)
        x[:-2] += 0.1
        eng.scan(x)                           # (warm-up: code objects, table slots)
        eng.pair_posteriors(x, 1e-3)
        _, pbest, pall = timed(lambda: eng.pair_posteriors(x, 1e-3), eng)
        eng.context_profiles(x)
        _, cbest, call_ = timed(lambda: eng.context_profiles(x), eng)
        eng.accessibility(x, width)
        acc, best, all_ms = timed(lambda: eng.accessibility(x, width), eng)
        mean = np.nanmean(np.concatenate(acc), axis=0)
        print(json.dumps(dict(pattern=pattern, n=n, L=L, U=width, call_ms=best[0][0], sums_and_access_kernels_ms=best[0][1],
                              log_space_sequences=best[0][2], call_ms_all=all_ms, host_wall_s=round(best[1], 3),
                              pair_call_ms=pbest[0][0], pair_sums_ms=pbest[0][1], pair_call_ms_all=pall,
                              context_call_ms=cbest[0][0], context_sums_ms=cbest[0][1], context_call_ms_all=call_,
                              ratio_to_pair_call=round(best[0][0] / pbest[0][0], 4),
                              ratio_to_context_call=round(best[0][0] / cbest[0][0], 4),
                              mean_access={"u%d" % (w + 1): round(float(v), 5) for w, v in enumerate(mean) if w + 1 in (1, 2, 4, 8, 16, 32, 64)})),
              flush=True)


if __name__ == "__main__":
    main()
