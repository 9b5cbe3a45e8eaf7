"""Hard structure constraints: wall time of load_batch of n x L three ways -- plain, with all-'.' strings
(constrained mode), with 'x' on 10 % of the positions --, three loads each.  k_constrain's own time comes from a separate
`rocprofv3 --kernel-trace --stats` run of this script.

    python tools/constraint_load.py n L"""
import os, sys, time
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
from rnaelem_amd import api, synth
n, L = int(sys.argv[1]), int(sys.argv[2])
pat = "(.....)"
eng = api.Engine(pat, "~T2004~", 50, 30, 1e-4, 0.1, 0, 0)
seqs, quals = synth.synth_batch(n, L, seed=77 + L)
free = ["." * L] * n
rng = np.random.default_rng(1)
xs = ["".join("x" if r < 0.1 else "." for r in rng.random(L)) for _ in range(n)]
constrained = hasattr(api.load_library(), "elemdp_load_batch_constrained")
for rep in range(3):
    for name, cons in (("plain", None), ("all-free strings", free), ("x on 10 %", xs)):
        if cons is not None and not constrained:
            continue
        t0 = time.perf_counter()
        if cons is None:
            eng.load_batch(seqs, quals)
        else:
            eng.load_batch(seqs, quals, constraints=cons)
        print("load_batch %d x %d, %s: %.3f s" % (n, L, name, time.perf_counter() - t0), flush=True)
