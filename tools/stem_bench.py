"""Pair posteriors by motif node pair under the motif model: device time of elemdp_stem_profile next to
elemdp_pair_posteriors and elemdp_node_profile of the same process, one after the other on the same batch, from the engine's HIP
events (last_timing: ms[0] the whole call with the copy of its result, ms[1] the sum passes + the call's own kernels); best of
three.  The pair call is the yardstick: the same sum passes, one reduction per cell.  The stem call is timed without a list
(min_prob = inf: counts alone) and with one (min_prob 0.01, as `scan --out-stem-pairs`).  Prints one JSON line per shape.

    python tools/stem_bench.py [n] [L ...]       (default: 10000 sequences of L = 200 and of L = 300, pattern ((.*.)))

The share of each kernel comes from a separate `rocprofv3 --kernel-trace --stats` run of this script: k_stem_cells, k_stem_counts,
k_stem_seq and k_list_scatter against k4_pairs / k_pair_seq and the sum passes (k4_in / k4_in_ext / k4_out_ext / k4_r7 / k4_out /
k5_pick)."""
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
    pattern = os.environ.get("STEM_BENCH_PATTERN", "((.*.))")
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
        eng.node_profiles(x)
        _, nbest, nall = timed(lambda: eng.node_profiles(x), eng)
        eng.stem_profiles(x)
        counts, best, all_ms = timed(lambda: eng.stem_profiles(x), eng)
        (_, lists), lbest, lall = timed(lambda: eng.stem_profiles(x, 0.01), eng)
        slots, names = eng.stem_slots(), eng.describe()["node"]
        logo = api.stem_logo(counts, slots, names)
        K = len(slots)
        print(json.dumps(dict(pattern=pattern, n=n, L=L, slots=K, kept_cells=kept,
                              staging_bound_bytes=kept * K * 17, list_entries=int(sum(len(l[3]) for l in lists)),
                              call_ms=best[0][0], sums_and_stem_kernels_ms=best[0][1], log_space_sequences=best[0][2], call_ms_all=all_ms,
                              host_wall_s=round(best[1], 3),
                              call_with_list_ms=lbest[0][0], sums_and_stem_kernels_with_list_ms=lbest[0][1], call_with_list_ms_all=lall,
                              pair_call_ms=pbest[0][0], pair_sums_and_kernels_ms=pbest[0][1], pair_call_ms_all=pall,
                              node_call_ms=nbest[0][0], node_sums_and_kernels_ms=nbest[0][1], node_call_ms_all=nall,
                              call_over_pair_call=round(best[0][0] / pbest[0][0], 4),
                              kernels_over_pair_kernels=round(best[0][1] / pbest[0][1], 4),
                              call_with_list_over_pair_call=round(lbest[0][0] / pbest[0][0], 4),
                              occurrences={l: round(float(v), 2) for l, v in zip(logo["labels"], logo["occurrences"])},
                              mutual_information={l: round(float(v), 4) for l, v in zip(logo["labels"], logo["mutual_information"])})),
              flush=True)


if __name__ == "__main__":
    main()
