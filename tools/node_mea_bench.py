"""Maximum expected accuracy motif alignments and site lists: device time of elemdp_node_mea without a
profile buffer (K = 1 and K = 4) next to elemdp_node_profile of the same process, from the engine's HIP events (last_timing:
ms[0] the whole call with the copies of its results, ms[1] the sum passes + the node kernels + the decode).  Prints one JSON line
per shape.

    python tools/node_mea_bench.py [n] [L ...]       (default: 10000 sequences of L = 200 and of L = 300, pattern ((.*.)))

A library without elemdp_node_mea (the parent of the change) gives the node_profiles figures alone.  The decode kernel's own time
comes from a separate `rocprofv3 --kernel-trace --stats` run of this script: k_node_mea against k_node_pos."""
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
    gamma = float(os.environ.get("NODE_MEA_GAMMA", "4"))
    has_mea = hasattr(api.Engine, "mea_alignments")
    for L in lengths:
        eng = api.Engine(pattern, "~T2004~", 50, 30, 1e-4, 0.1, 0, 0)
        seqs, quals = synth.synth_batch(n, L, seed=L)
        eng.load_batch(seqs, quals)
        x = eng.initial_params(1.0)
        x[:-2] += 0.1
        eng.scan(x)                           # (warm-up: code objects, table slots)
        eng.node_profiles(x)
        _, nbest, nall = timed(lambda: eng.node_profiles(x), eng)
        out = dict(pattern=pattern, n=n, L=L, node_profile_call_ms=nbest[0][0], node_profile_sums_and_kernel_ms=nbest[0][1],
                   node_profile_call_ms_all=nall, node_profile_host_wall_s=round(nbest[1], 3))
        if has_mea:
            out["gamma"] = gamma
            for K in (1, 4):
                eng.mea_alignments(x, gamma, K)
                res, best, all_ms = timed(lambda: eng.mea_alignments(x, gamma, K), eng)
                out["mea_K%d" % K] = dict(call_ms=best[0][0], sums_node_kernels_and_decode_ms=best[0][1], log_space_sequences=best[0][2],
                                         call_ms_all=all_ms, host_wall_s=round(best[1], 3),
                                         sites=int(sum(len(r["start"]) for r in res)),
                                         sequences_with_a_site=int(sum(len(r["start"]) > 0 for r in res)))
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
