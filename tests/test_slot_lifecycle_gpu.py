"""The life cycle of the table slots on one handle (TableSlots): train evaluations, scans of both pipelines,
option changes that resize or invalidate the slots, ranged evaluations, loads of other batches and the table export follow each
other, and every result is what a fresh handle with the same options and batch gives -- to the bit for the deterministic train
evaluations, as tests/test_pair_posterior_gpu.py compares scans for the scans."""
import numpy as np
import pytest

from rnaelem_amd import api, synth

pytestmark = pytest.mark.gpu

PAR = "~T2004~"
PATTERN = "((.*.))"


def batch(lengths, seed):
    seqs, quals = [], []
    for L in lengths:
        s, q = synth.synth_batch(1, L, seed=seed + L)
        seqs += s
        quals += q
    for k in range(0, len(quals), 2):
        quals[k][-1] = 5
    return seqs, quals


def engine(options):
    eng = api.Engine(PATTERN, PAR, 50, 30, 1e-4, 0.1, 0, 0)
    for key, v in options.items():
        eng.set_option(key, v)
    return eng


def same_scan(got, ref):
    (ra, ea), (rb, eb) = ref, got
    np.testing.assert_allclose(eb, ea, rtol=1e-13, atol=1e-300)
    assert len(ra) == len(rb)
    for p, q in zip(ra, rb):     # (the scan's posteriors are summed with atomics: equal to the last bits)
        assert (p["Ys"], p["Ye"], p["rss"]) == (q["Ys"], q["Ye"], q["rss"]) and np.array_equal(p["psihat"], q["psihat"])
        assert q["exist_prob"] == pytest.approx(p["exist_prob"], rel=1e-13)
        for key in ("start", "inner", "end"):
            assert np.array_equal(np.isfinite(p[key]), np.isfinite(q[key])), key
            np.testing.assert_allclose(q[key], p[key], rtol=1e-13, atol=1e-13, err_msg=key)


def same_train(got, ref):
    assert got[0] == ref[0] and np.array_equal(got[1], ref[1]) and got[2:] == ref[2:]


def test_slots_through_the_life_of_a_handle():
    first = batch((20, 27, 33, 38, 44, 51, 57, 60), 300)
    longer = batch((35, 90, 48, 71, 22), 500)
    single = batch((40,), 700)
    opts = {"deterministic": 1}
    eng = engine(opts)
    x = eng.initial_params(0.7)
    x[:-2] += np.linspace(-0.3, 0.3, len(x) - 2)
    x[-1] += 0.2
    fresh_cache = {}

    def fresh(what, loaded, rng=None):
        """what a handle that has done nothing else gives: the options of now, set before its one load"""
        key = (what, id(loaded), rng, tuple(sorted(opts.items())))
        if key not in fresh_cache:
            e = engine(opts)
            e.load_batch(*loaded)
            if rng:
                e.set_option("eval_first", rng[0])
                e.set_option("eval_count", rng[1])
            fresh_cache[key] = e.scan(x) if what == "scan" else e.train_eval(x)
        return fresh_cache[key]

    def option(key, v):
        eng.set_option(key, v)
        opts[key] = v

    def train(loaded, rng=None):
        same_train(eng.train_eval(x), fresh("train", loaded, rng))

    eng.load_batch(*first)
    train(first)                                          # 1
    option("pipeline", 3)                                 # 2: the fused scan kernel on slots with trace tables
    same_scan(eng.scan(x), fresh("scan", first))
    option("pipeline", 4)
    train(first)                                          # 3
    option("prune", 0)                                    # 4
    train(first)                                          # 5
    option("prune", 1)                                    # 6
    option("group", 2)
    train(first)                                          # 7
    option("group", 0)                                    # 8
    train(first)                                          # 9
    eng.set_option("eval_first", 2)                       # 10: a range, then the whole batch
    eng.set_option("eval_count", 3)
    train(first, (2, 3))
    eng.set_option("eval_first", 0)
    eng.set_option("eval_count", 0)
    train(first)
    eng.load_batch(*longer)                               # 11
    train(longer)                                         # 12
    eng.load_batch(*first)                                # 13
    same_scan(eng.scan(x), fresh("scan", first))          # 14
    train(first)
    eng.load_batch(*single)                               # 15
    train(single)
    ref = engine(opts)
    ref.load_batch(*single)
    ref.train_eval(x)
    want, got = ref.debug_tables(), eng.debug_tables()
    assert set(got) == set(want)
    for key in want:
        assert np.array_equal(np.isfinite(got[key]), np.isfinite(want[key])), key
        np.testing.assert_allclose(got[key], want[key], rtol=1e-13, atol=0, err_msg=key)
    # the sum passes of a scan leave nothing the export can read: it refuses until the next train evaluation
    eng.scan(x)
    with pytest.raises(api.ElemdpError, match="debug_tables before train_eval"):
        eng.debug_tables()
    train(single)
    eng.debug_tables()
