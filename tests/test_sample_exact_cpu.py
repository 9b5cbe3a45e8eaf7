"""The sampler's log-probabilities, exactly, on the CPU: every sample of the CPU driver (tests/sample_emul.cpp,
the rule of sample_rules.h on the product's inside rules) reports logp == Oracle.derivation_logz(rss, nodes) - Zo, the weight of
that one derivation in the oracle's own recursion over the partition function.  A wrong weight in one rule of
sample_candidates, which the sample frequencies of tests/test_sample_cpu.py cannot resolve, moves logp by its full size here.
Also: the structure level (frequencies and sums of logp against the fixed-structure partition function), the constraint of
derivation_logz itself, and the refusal path of the walk's stack bound."""
import itertools

import numpy as np
import pytest

from oracle import pyoracle as po
from rnaelem_amd import api, io, synth
from tests.sample_check import (Driver, bound, check_exact_logp, distinct, dot_bracket, driver_from_model, logp_atol, motif_span,
                                oracle_map, oracle_zo, stack_cap)
from tests.test_pair_posterior_gpu import PAR, PATTERNS, perturbed, ragged_batch
from tests.test_pair_shapes_gpu import P1, batch, edge_batch, oracle_maker
from tests.util import gpath

N_DRAWN = 130      # samples per sequence; up to MAX_CHECK distinct ones are checked, always sample 0 and the last one
MAX_CHECK = 64


def picks_of(rss, nodes):
    groups = distinct(rss, nodes)
    first = [ts[0] for ts in groups.values()]
    last = len(rss) - 1
    keep = first[:MAX_CHECK - 1]
    return sorted(set(keep) | {0, last})


def exact_case(drv, make_oracle, seqs, quals, x, seed, what, fasts=(False, True)):
    """both forms of the driver's inside tables: every picked sample exact; returns the worst |logp - oracle| / max(1, |Zo|)"""
    Zo = oracle_zo(make_oracle, seqs, quals)
    worst = 0.0
    for fast in fasts:
        drv.set_fast(fast)
        samples, picks = [], []
        for k, (s, q) in enumerate(zip(seqs, quals)):
            r = drv.sample(x, s, q, N_DRAWN, seed, k)
            samples.append(r)
            if not np.isfinite(Zo[k]):
                assert r[3] == 1, (what, k)
                picks.append([])
                continue
            assert r[3] == 0 and np.all(np.isfinite(r[2])), (what, k, r[3])
            picks.append(picks_of(r[0], r[1]))
        worst = max(worst, check_exact_logp(make_oracle, seqs, quals, Zo, samples, picks, what=(what, "fast", fast)))
    print("exact logp %s: worst |logp - oracle| / max(1, |Zo|) = %.3g" % (what, worst))
    return Zo, samples


@pytest.mark.parametrize("pattern", PATTERNS)
def test_logp_is_the_weight_of_the_derivation(pattern):
    seqs, quals = ragged_batch()
    x = perturbed(api.Engine(pattern, PAR, 50, 30, 1e-4, 0.1, 0, 0))
    exact_case(Driver(pattern, PAR), oracle_maker(pattern, 50, 30, x), seqs, quals, x, 7, pattern)


@pytest.mark.parametrize("W,C", [(20, 5), (33, 30), (100, 30), (300, 30)])
def test_logp_at_other_band_widths(W, C):
    """L = 1, 2, and L = 5 unless its ends pair and the filter keeps that cell, hold one derivation (every base exterior and
    before the motif): logp = 0"""
    seqs, quals = batch([1, 2, 5, W - 1, W, W + 1, 2 * W + 7], seed=1000 * W + C)
    x = perturbed(api.Engine(P1, PAR, W, C, 1e-4, 0.1, 0, 0))
    _, samples = exact_case(Driver(P1, PAR, W, C), oracle_maker(P1, W, C, x), seqs, quals, x, 11, (W, C))
    o = oracle_maker(P1, W, C, x)()
    for k in range(3):
        rss, nodes, logp, st = samples[k]
        if k == 2 and o.bpp(seqs[k])[1].sum() > 0:
            continue
        assert len(distinct(rss, nodes)) == 1 and np.all(np.abs(logp) <= 1e-12), (k, logp[:3])


@pytest.mark.parametrize("pattern", ["(.........)", P1])
def test_logp_of_edge_sequences(pattern):
    """all N, poly-A, L = 1 and 2 keep no pair: one structure; with `(.........)` GGGAAAUCCC has no room for the motif"""
    seqs, quals = edge_batch()
    x = perturbed(api.Engine(pattern, PAR, 50, 30, 1e-4, 0.1, 0, 0))
    exact_case(Driver(pattern, PAR), oracle_maker(pattern, 50, 30, x), seqs, quals, x, 13, pattern)


@pytest.mark.parametrize("model", ["syn_sm.model", "syn_a2007.model", "syn_c12.model", "tiny_a.model", "1.model", "2.model"])
def test_logp_under_other_models(model):
    """softmax theta, ~A2007~, W 40 / C 12, W 30, W 20 / C 999 and --no-rss (2.model: the driver runs it; every structure is
    all O there, rule 8 alone, and only the alignment varies)"""
    m = io.read_model(gpath(model))
    seqs, quals = batch((3, 13, 40, 97, 131, 200), seed=len(model))
    _, samples = exact_case(driver_from_model(m), lambda: po.oracle_from_model(gpath(model))[0], seqs, quals, m["x"], 17, model)
    if m["no_rss"]:
        o = po.oracle_from_model(gpath(model))[0]
        for (rss, nodes, logp, st), s, q in zip(samples, seqs, quals):
            assert all(r == "O" * len(s) for r in rss)
            sc = o.scan_seq(s, q)          # (the oracle's best parse too, where it has one with the motif)
            assert sc["rss"] == ("O" if sc["exist_prob"] > 0.0 else " ") * len(s)
            assert len(distinct(rss, nodes)) > 1 or len(s) < 10


@pytest.mark.parametrize("pattern", ["((.*.))", "(.....)"])
def test_structure_frequencies_and_sums_against_the_fixed_structure_oracle(pattern):
    """N = 4000 on the sequences with L <= 40: a structure drawn at least 50 times has its frequency within `bound` of
    exp(Zo_fix(r) - Zo); the logp of the distinct alignments of a structure sum to at most that; all distinct samples to at
    most 1.  Zo_fix from the oracle's own fix_rss switch (ORC_DBG_FIX_RSS), and derivation_logz without nodes agrees with it."""
    N = 4000
    seqs, quals = ragged_batch()
    x = perturbed(api.Engine(pattern, PAR, 50, 30, 1e-4, 0.1, 0, 0))
    drv = Driver(pattern, PAR)
    make = oracle_maker(pattern, 50, 30, x)

    def make_fix():
        o = po.make_oracle(pattern, 50, 30, min_bpp=1e-4, tau=0.1, flags=po.DBG_FIX_RSS)
        o.set_params(x)
        return o

    o = make()
    checked = 0
    for k, (s, q) in enumerate(zip(seqs, quals)):
        if len(s) > 40:
            continue
        Zo = o.train_seq(s, q)["Zo"]
        tol = logp_atol(Zo)
        rss, nodes, logp, st = drv.sample(x, s, q, N, 7, k)
        assert st == 0
        by_struct = {}
        for (r, h), ts in distinct(rss, nodes).items():
            by_struct.setdefault(dot_bracket(r), []).append(ts)
        dbs = list(by_struct)
        zfix = oracle_map(make_fix, lambda of, db: of.train_seq(s, q, fix_rss=db)["Zo"], dbs)
        for db, zf in zip(dbs, zfix):
            assert o.derivation_logz(s, q, db, None) == zf, (k, db)
            count = sum(len(ts) for ts in by_struct[db])
            p = np.exp(zf - Zo)
            if count >= 50:
                assert abs(count / N - p) <= bound(p, N), (pattern, k, db, count / N, p)
                checked += 1
            lse = np.logaddexp.reduce([logp[ts[0]] for ts in by_struct[db]])
            assert lse <= zf - Zo + tol, (pattern, k, db, lse, zf - Zo)
        total = sum(np.exp(logp[ts[0]]) for ts in distinct(rss, nodes).values())
        assert total <= 1.0 + tol, (pattern, k, total)
    assert checked >= 2


def alignments(L, names):
    """every node row of the shape z* n1+ n2+ .. o* (the motif placed anywhere, each of its nodes on one or more positions: a
    '.' node repeats at the price of tau, and so does a bracket node along a stem), and the row without the motif; most of
    them fit no derivation of a given structure and weigh nothing"""
    M = len(names)
    inner = list(range(1, M - 1))
    yield np.zeros(L, dtype=np.uint8)
    for m in range(len(inner), L + 1):
        for split in itertools.combinations_with_replacement(range(len(inner)), m - len(inner)):
            reps = [1] * len(inner)
            for d in split:
                reps[d] += 1
            body = [h for h, n in zip(inner, reps) for _ in range(n)]
            for a in range(0, L - m + 1):
                yield np.array([0] * a + body + [M - 1] * (L - m - a), dtype=np.uint8)


def test_node_constraint_selects_single_derivations_that_sum_to_the_structure():
    """`(.....)` on the L = 13 sequence: over every alignment of the motif (or none), exp(derivation_logz) sums to
    exp(Zo_fix(r)) of the oracle's own fix_rss switch, for the sampled structures and for the open chain; and a node the pattern
    cannot place at a position gives -inf."""
    pattern = "(.....)"
    seqs, quals = ragged_batch()
    s, q = seqs[0], quals[0]
    L = len(s)
    assert L <= 13
    eng = api.Engine(pattern, PAR, 50, 30, 1e-4, 0.1, 0, 0)
    x = perturbed(eng)
    names = eng.describe()["node"]
    M = len(names)
    o = oracle_maker(pattern, 50, 30, x)()
    of = po.make_oracle(pattern, 50, 30, min_bpp=1e-4, tau=0.1, flags=po.DBG_FIX_RSS)
    of.set_params(x)
    assert o.derivation_logz(s, q, None, None) == o.train_seq(s, q)["Zo"]
    rss, nodes, logp, st = Driver(pattern, PAR).sample(x, s, q, 500, 7, 0)
    structs = sorted({dot_bracket(r) for r in rss} | {"." * L})
    assert len(structs) >= 3
    rows = list(alignments(L, names))
    with_motif = 0
    for db in structs:
        z = np.array([o.derivation_logz(s, q, db, h) for h in rows])
        with_motif += int(np.isfinite(z[1:]).sum())
        zf = of.train_seq(s, q, fix_rss=db)["Zo"]
        assert np.exp(z).sum() == pytest.approx(np.exp(zf), rel=1e-12), db
    assert with_motif > 0
    for r, h in zip(rss[:50], nodes[:50]):
        a, b = motif_span(h, M)
        bad = h.copy()
        bad[a if a >= 0 else 0] = M - 1          # ('o' in front of a motif node or of 'z')
        if a < 0 and L == 1:
            continue
        assert np.isfinite(o.derivation_logz(s, q, dot_bracket(r), h))
        assert o.derivation_logz(s, q, dot_bracket(r), bad) == -np.inf


def hairpin(h):
    return np.array([3] * h + [1, 1, 1, 1] + [2] * h, dtype=np.uint8)


def refusal_sequences():
    enc = {"A": 1, "C": 2, "G": 3, "U": 4}
    chain = np.array([enc[c] for c in "GGGAAAACCC" * 12], dtype=np.uint8)
    (rnd,), _ = synth.synth_batch(1, 200, seed=41)
    return {"GGGAAAACCC x 12": chain, "G^23 AAAA C^23": hairpin(23), "random L = 200": rnd}


def test_a_walk_beyond_its_stack_bound_is_refused_and_the_bound_is_never_met():
    """The walk checks `top + 3 > cap` after it pops a target, so with cap = 3 it goes on only while no second frame is pending:
    that admits the open chain and a first stem that starts at base 0, nothing else.  On A + G^h AAAA C^h (base 0 pairs with
    nothing, the stem is worth e^-20 and more) every one of 500 samples is refused: status 2, blank letters, node 0, NaN logp.
    On the ragged batch a sample under cap = 3 is blank or the sample of the full stack.  The smallest cap at which all 500 walks
    complete is far below sample_stack_cap(L) = L + 4 (printed; DESIGN.md section 14 quotes them)."""
    pattern = "((.*.))"
    x = perturbed(api.Engine(pattern, PAR, 50, 30, 1e-4, 0.1, 0, 0))
    drv = Driver(pattern, PAR)
    for h in (8, 23):
        s = np.concatenate([[1], hairpin(h)]).astype(np.uint8)
        q = np.full(len(s) + 1, 10, dtype=np.uint8)
        assert len(s) >= 10
        rss, nodes, logp, st = drv.sample(x, s, q, 500, 3, 0, cap=3)
        assert st == 2
        assert all(r == " " * len(s) for r in rss) and not nodes.any() and np.all(np.isnan(logp))
    seqs, quals = ragged_batch()
    for k, (s, q) in enumerate(zip(seqs, quals)):
        full = drv.sample(x, s, q, 200, 3, k)
        rss, nodes, logp, st = drv.sample(x, s, q, 200, 3, k, cap=3)
        refused = 0
        for t in range(200):
            if np.isnan(logp[t]):
                refused += 1
                assert rss[t] == " " * len(s) and not nodes[t].any()
            else:
                assert rss[t] == full[0][t] and np.array_equal(nodes[t], full[1][t]) and logp[t] == full[2][t]
                assert "R" not in rss[t] or rss[t][0] == "L"
        assert st == (2 if refused else 0) and (refused > 100 or len(s) < 40), (k, refused)
    for name, s in refusal_sequences().items():
        q = np.full(len(s) + 1, 10, dtype=np.uint8)
        L = len(s)
        assert drv.sample(x, s, q, 500, 5, 0)[3] == 0
        lo, hi = 1, stack_cap(L)           # (complete at hi; the walks that complete at a cap complete at every larger one)
        while lo < hi:
            mid = (lo + hi) // 2
            if drv.sample(x, s, q, 500, 5, 0, cap=mid)[3] == 0:
                hi = mid
            else:
                lo = mid + 1
        print("smallest stack cap for 500 walks, %s (L = %d): %d (sample_stack_cap %d)" % (name, L, lo, stack_cap(L)))
        assert lo <= stack_cap(L)
        assert drv.sample(x, s, q, 500, 5, 0, cap=lo - 1)[3] == 2
