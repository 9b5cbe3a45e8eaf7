"""Motif-conditional pair posteriors: device time of elemdp_pair_conditional -- without structures, and with
both MEA structures at gamma = 1 -- next to elemdp_pair_posteriors of the same process, all at min_prob 1e-3, from the engine's HIP
events (last_timing: ms[0] the whole call, ms[1] the sweeps + reductions + decodes).  Prints one JSON line per shape.

    python tools/cond_bench.py [n] [L ...]       (default: 10000 sequences of L = 200, pattern ((.*.)))

The new call runs one inside and two outside sweeps where two pair calls run two of each: ms[0] of the call without structures
has to stay below twice ms[0] of the pair call of the same run."""
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
    lengths = [int(v) for v in args[1:]] or [200]
    pattern = os.environ.get("COND_BENCH_PATTERN", "((.*.))")
    for L in lengths:
        eng = api.Engine(pattern, "~T2004~", 50, 30, 1e-4, 0.1, 0, 0)
        seqs, quals = synth.synth_batch(n, L, seed=L)
        eng.load_batch(seqs, quals)
        x = eng.initial_params(1.0)
        x[:-2] += 0.1
        eng.scan(x)                           # (warm-up: code objects, table slots)
        eng.pair_posteriors(x, 1e-3)
        eng.conditional_pairs(x, 1e-3, 1.0)
        prs, pbest, pall = timed(lambda: eng.pair_posteriors(x, 1e-3), eng)
        out = dict(pattern=pattern, n=n, L=L, min_prob=1e-3, pair_call_ms=pbest[0][0], pair_sums_and_kernels_ms=pbest[0][1],
                   pair_call_ms_all=pall, pairs_listed=int(sum(len(r[0]) for r in prs)))
        for name, gamma in (("cond", None), ("cond_gamma1", 1.0)):
            res, best, all_ms = timed(lambda: eng.conditional_pairs(x, 1e-3, gamma), eng)
            out[name] = dict(call_ms=best[0][0], sweeps_reductions_decodes_ms=best[0][1], log_space_sequences=best[0][2],
                             call_ms_all=all_ms, host_wall_s=round(best[1], 3), pairs_listed=int(sum(len(r["i"]) for r in res)),
                             mean_exist_prob=float(sum(r["exist_prob"] for r in res) / len(res)),
                             mean_shift=float(sum(r["shift"] for r in res if r["shift"] == r["shift"]) / len(res)))
        out["cond_over_pair"] = out["cond"]["call_ms"] / out["pair_call_ms"]
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
