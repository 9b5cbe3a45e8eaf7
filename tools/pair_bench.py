"""Base-pair posteriors under the motif model: device time of elemdp_pair_posteriors next to a scan of the
same batch, from the engine's HIP events (last_timing).  Prints one JSON line per shape.

    python tools/pair_bench.py [--mea] [--samples K[,K..]] [n] [L ...]   (default: 10000 sequences of L = 200 and of L = 300,
                                                                         pattern ((.*.)))

--mea: each shape also times elemdp_pair_mea (gamma 1, the same min_prob) on the same batch, right after the pair calls
(DESIGN.md section 13); k_pair_mea's share of that call comes from the kernel trace.
--samples K: each shape also times elemdp_sample with K samples per sequence; k_sample's own device time
comes from the kernel trace of a run with option group_streams 1 (PAIR_BENCH_GROUP_STREAMS=1).

The pair kernels' share of the call comes from a separate `rocprofv3 --kernel-trace --stats` run of this script: k4_pairs,
k_pair_seq, k_pair_kept, k_pair_prefix and k_list_scatter against the sum passes (k4_in / k4_in_ext / k4_out_ext / k4_r7 /
k4_out / k5_pick)."""
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
    mea = "--mea" in args
    args = [a for a in args if a != "--mea"]
    samples = []
    if "--samples" in args:
        k = args.index("--samples")
        samples = [int(v) for v in args[k + 1].split(",")]
        del args[k:k + 2]
    n = int(args[0]) if args else 10000
    lengths = [int(v) for v in args[1:]] or [200, 300]
    pattern = os.environ.get("PAIR_BENCH_PATTERN", "((.*.))")
    for L in lengths:
        eng = api.Engine(pattern, "~T2004~", 50, 30, 1e-4, 0.1, 0, 0)
        if os.environ.get("PAIR_BENCH_GROUP_STREAMS"):
            eng.set_option("group_streams", int(os.environ["PAIR_BENCH_GROUP_STREAMS"]))
        seqs, quals = synth.synth_batch(n, L, seed=L)
        eng.load_batch(seqs, quals)
        x = eng.initial_params(1.0)
        x[:-2] += 0.1
        eng.scan(x)                           # (warm-up: code objects, table slots)
        eng.pair_posteriors(x, 1e-3)
        res, best, all_ms = timed(lambda: eng.pair_posteriors(x, 1e-3), eng)
        out = {}
        if mea:
            eng.mea_structures(x, 1.0, 1e-3)
            (structs, _, _), mb, mall = timed(lambda: eng.mea_structures(x, 1.0, 1e-3), eng)
            out = dict(mea_call_ms=mb[0][0], mea_sums_and_pair_kernels_ms=mb[0][1], mea_call_ms_all=mall,
                       mea_host_wall_s=round(mb[1], 3), mea_paired_bases=sum(len(s) - s.count(".") for s in structs))
        for K in samples:
            eng.sample_structures(x, K)
            _, sb, sall = timed(lambda: eng.sample_structures(x, K), eng)
            out["sample_%d_call_ms" % K] = sb[0][0]
            out["sample_%d_call_ms_all" % K] = sall
            out["sample_%d_host_wall_s" % K] = round(sb[1], 3)
        eng.scan(x)
        scan_ms = eng.last_timing()[0]
        n_pairs = sum(len(r[2]) for r in res)
        print(json.dumps(dict(pattern=pattern, n=n, L=L, call_ms=best[0][0], sums_and_pair_kernels_ms=best[0][1],
                              log_space_sequences=best[0][2], call_ms_all=all_ms,
                              host_wall_s=round(best[1], 3), scan_ms=scan_ms, pairs_ge_1e_3=n_pairs, **out)), flush=True)


if __name__ == "__main__":
    main()
