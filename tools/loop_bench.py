"""Loop posteriors under the motif model: device time of elemdp_loop_posteriors next to
elemdp_pair_posteriors of the same process, one after the other on the same batch, from the engine's HIP events (last_timing:
ms[0] the whole call with the scatter of its lists, ms[1] the sum passes + the call's own kernels); best of three.  The pair call
is the yardstick: the same sum passes, one reduction per cell.  The loop call is timed with min_prob 0.01 without the counts (as
`scan --out-loops` lists: only the cells whose pair posterior reaches 0.01 are walked), with min_prob 0.01 and the counts (every
kept cell is walked) and with min_prob 0 (every kept cell walked and listed).  Prints one JSON line per shape.

    python tools/loop_bench.py [n] [L ...]       (default: 10000 sequences of L = 200 and of L = 300, pattern ((.*.)))

The share of each kernel comes from a separate `rocprofv3 --kernel-trace --stats` run of this script: k4_pairs, k_helix_units,
k_loop_unary, k_loop_items, k_loop_seq and k_loop_scatter against k_pair_seq and the sum passes (k4_in / k4_in_ext / k4_out_ext /
k4_r7 / k4_out / k5_pick)."""
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
    pattern = os.environ.get("LOOP_BENCH_PATTERN", "((.*.))")
    for L in lengths:
        eng = api.Engine(pattern, "~T2004~", 50, 30, 1e-4, 0.1, 0, 0)
        seqs, quals = synth.synth_batch(n, L, seed=L)
        eng.load_batch(seqs, quals)
        x = eng.initial_params(1.0)
        x[:-2] += 0.1
        eng.scan(x)                           # (warm-up: code objects, table slots)
        full = eng.pair_posteriors(x, 0.0)
        kept = sum(len(r[0]) for r in full)
        eng.pair_posteriors(x, 1e-3)
        _, pbest, pall = timed(lambda: eng.pair_posteriors(x, 1e-3), eng)
        eng.loop_posteriors(x, 0.01, counts=False)
        res, best, all_ms = timed(lambda: eng.loop_posteriors(x, 0.01, counts=False), eng)
        _, bestc, allc = timed(lambda: eng.loop_posteriors(x, 0.01), eng)
        res0, best0, all0 = timed(lambda: eng.loop_posteriors(x, 0.0), eng)
        print(json.dumps(dict(pattern=pattern, n=n, L=L, kept_cells=kept, items=int(sum(len(t[4]) for t in res0[1])),
                              min_prob=0.01, closing_entries=int(sum(len(c[2]) for c in res[0])),
                              two_loop_entries=int(sum(len(t[4]) for t in res[1])),
                              call_ms=best[0][0], sums_and_loop_kernels_ms=best[0][1], log_space_sequences=best[0][2], call_ms_all=all_ms,
                              host_wall_s=round(best[1], 3),
                              call_with_counts_ms=bestc[0][0], sums_and_loop_kernels_with_counts_ms=bestc[0][1], call_with_counts_ms_all=allc,
                              call_at_0_ms=best0[0][0], sums_and_loop_kernels_at_0_ms=best0[0][1], call_at_0_ms_all=all0,
                              pair_call_ms=pbest[0][0], pair_sums_and_kernels_ms=pbest[0][1], pair_call_ms_all=pall,
                              call_over_pair_call=round(best[0][0] / pbest[0][0], 4),
                              kernels_over_pair_kernels=round(best[0][1] / pbest[0][1], 4),
                              kernels_minus_pair_kernels_ms=round(best[0][1] - pbest[0][1], 3),
                              call_with_counts_over_pair_call=round(bestc[0][0] / pbest[0][0], 4),
                              call_at_0_over_pair_call=round(best0[0][0] / pbest[0][0], 4),
                              kernels_at_0_minus_pair_kernels_ms=round(best0[0][1] - pbest[0][1], 3))),
              flush=True)


if __name__ == "__main__":
    main()
