"""Scan posteriors in one world: device time of the context, accessibility, loop and pair calls in world 0
(mixture), 1 (motif) and 2 (none), next to elemdp_pair_conditional of the same process, from the engine's HIP events (last_timing:
ms[0] the whole call, ms[1] its sweeps and kernels, [2] sequences handed to the log-space form), best of three by ms[1].  Prints one JSON line
per shape.

    python tools/world_bench.py [n] [L ...]       (default: 10000 sequences of L = 200, pattern ((.*.)))

A world call runs one inside and one outside sweep, the conditional call one outside sweep more: ms[1] of the pair call in world 1
has to stay below ms[1] of the conditional call of the same run."""
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from rnaelem_amd import api, synth  # noqa: E402


def timed(call, eng):
    reps = []
    for _ in range(3):
        call()
        reps.append(eng.last_timing().tolist())
    return min(reps, key=lambda r: r[1]), [r[1] for r in reps]      # (best by ms[1], the figure that is compared)


def main():
    args = sys.argv[1:]
    n = int(args[0]) if args else 10000
    lengths = [int(v) for v in args[1:]] or [200]
    pattern = os.environ.get("WORLD_BENCH_PATTERN", "((.*.))")
    for L in lengths:
        eng = api.Engine(pattern, "~T2004~", 50, 30, 1e-4, 0.1, 0, 0)
        seqs, quals = synth.synth_batch(n, L, seed=L)
        eng.load_batch(seqs, quals)
        x = eng.initial_params(1.0)
        x[:-2] += 0.1
        calls = dict(pairs=lambda w: eng.pair_posteriors(x, 1e-3, world=w), context=lambda w: eng.context_profiles(x, world=w),
                     access=lambda w: eng.accessibility(x, 16, world=w), loops=lambda w: eng.loop_posteriors(x, 0.01, world=w))
        eng.scan(x)                           # (warm-up: code objects, table slots)
        eng.conditional_pairs(x, 1e-3)
        for name in calls:
            calls[name]("motif")
        best, all_ms = timed(lambda: eng.conditional_pairs(x, 1e-3), eng)
        out = dict(pattern=pattern, n=n, L=L, cond=dict(call_ms=best[0], kernels_ms=best[1], log_space_sequences=best[2], kernels_ms_all=all_ms))
        for name, call in calls.items():
            out[name] = {}
            for w in api.WORLDS:
                best, all_ms = timed(lambda: call(w), eng)
                out[name][w] = dict(call_ms=best[0], kernels_ms=best[1], log_space_sequences=best[2], kernels_ms_all=all_ms)
            for w in api.WORLDS[1:]:
                out[name][w]["over_mixed"] = out[name][w]["kernels_ms"] / out[name]["mixed"]["kernels_ms"]
        out["pairs_motif_kernels_below_cond"] = out["pairs"]["motif"]["kernels_ms"] < out["cond"]["kernels_ms"]
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
