"""Hard structure constraints on the GPU: the mask of a constrained load against the brute force of
constraint_check.apply over the filter's mask; an all-free load against a plain one; the constrained ensemble of the enumerated
cases (train evaluation, pair posteriors, context, accessibility) against brute-force enumeration with the oracle; the
conditioning identities exp(ln Z_c - ln Z) = P(event) and the partition identity X_free = a X_x + (1 - a) X_| at larger shapes,
with references from the oracle alone; the sampler and the CYK structure; a whole structure given back as a string; the train
switches; the refusals; `scan --constraints` in chunks and over two ranks against one constrained load."""
import re

import numpy as np
import pytest

from oracle import pyoracle as po
from rnaelem_amd import api, cli, io, synth
from tests import access_check as ac
from tests import constraint_check as kc
from tests import ctx_check as cc
from tests import helix_check as hc
from tests import large_automata as la
from tests import loop_check as lc
from tests import node_check as nc
from tests.sample_check import logp_atol
from tests.pair_check import oracle_pairs, unpaired_of
from tests.test_pair_posterior_gpu import perturbed
from tests.train_check import GR_TOL, ROW_ATOL, ROW_RTOL
from tests.util import assert_log_close

pytestmark = pytest.mark.gpu

PAR = "~T2004~"
P1 = "((.*.))"
NARROW = (1, 5, 19, 20, 21, 47)                       # at max_span 20
WIDE = (107, 13, 64, 51, 50, 99, 33, 80, 107)         # nine sequences at max_span 50
SWITCHES = ("useful_mask", "loop_prepass", "loop_outside", "pair_terms", "live_blocks", "own_slots")


def shape_batch(lens, seed):
    seqs, quals = [], []
    for k, L in enumerate(lens):
        (s,), (q,) = synth.synth_batch(1, L, seed=seed + 17 * k + L)
        if k % 2:
            q[-1] = 5
        seqs.append(s)
        quals.append(q)
    return seqs, quals


def shape_strings(seqs, W, seed, kept=None):
    """one random string per sequence (the first stays free); with kept, forced pairs are pairs of those masks"""
    out = []
    for k, s in enumerate(seqs):
        L = len(s)
        rng = np.random.default_rng(seed + k)
        out.append(None if k == 0 else kc.random_string(rng, s, L, min(L, W), kept=None if kept is None else kept[k], p_single=0.1))
    return out


def structure_strings(seqs, quals, W, seed):
    """(strings, x): per sequence a string drawn from the CYK structure of its free fold, which satisfies it (None where the free
    scan has no parse)"""
    free = api.Engine(P1, PAR, W, 30, 1e-4, 0.1, 0, 0)
    free.load_batch(seqs, quals)
    x = perturbed(free)
    cons = []
    for k, r in enumerate(free.scan(x)[0]):
        rng = np.random.default_rng(seed + k)
        cons.append(None if not r["rss"].strip() else kc.string_from_structure(rng, kc.letters_to_db(r["rss"])))
    assert sum(c is not None and "(" in c for c in cons) >= 2 and sum(c is not None and c.strip(".()") != "" for c in cons) >= 2
    return cons, x


def pair_matrix(entry, L, W):
    ii, jj, pp, _ = entry
    P = np.zeros((L + 1, W + 1))
    P[ii, jj - ii] = pp
    return P


# ---- 1. the mask

@pytest.mark.parametrize("lens,W", [(NARROW, 20), (WIDE, 50)], ids=["narrow", "wide"])
@pytest.mark.parametrize("group", [1, 3])
def test_mask_of_a_constrained_load_equals_the_brute_force(lens, W, group):
    seqs, quals = shape_batch(lens, 300)
    free = api.Engine(P1, PAR, W, 30, 1e-4, 0.1, 0, 0)
    free.load_batch(seqs, quals)
    cons = shape_strings(seqs, W, 40)
    assert sum(c is not None and "(" in c for c in cons) >= 1 and sum(c is not None for c in cons) >= len(seqs) - 1
    eng = api.Engine(P1, PAR, W, 30, 1e-4, 0.1, 0, 0)
    eng.set_option("group", group)
    eng.load_batch(seqs, quals, constraints=cons)
    np.testing.assert_array_equal(eng.bpp_eff(), free.bpp_eff())          # (the filter sees no constraint)
    for k, s in enumerate(seqs):
        L = len(s)
        kept = free.pairs(k)[0]
        ref, _ = kc.apply(kept, s, cons[k] or "." * L, L, min(L, W))
        assert np.array_equal(eng.pairs(k)[0], ref), (k, L, cons[k])
    x = perturbed(eng)
    eng.train_eval(x)          # (the plan of the constrained mask serves an evaluation)


@pytest.mark.parametrize("lens,W", [(NARROW, 20), (WIDE, 50)], ids=["narrow", "wide"])
def test_streamed_batch_applies_the_strings_per_chunk_and_caches_the_filters_mask(lens, W):
    """(strings drawn from the CYK structures of the free fold: every constrained sequence keeps a parse, so the comparison is
    not one of zeros)"""
    seqs, quals = shape_batch(lens, 300)
    cons, x = structure_strings(seqs, quals, W, 70)
    res = api.Engine(P1, PAR, W, 30, 1e-4, 0.1, 0, 0)
    res.load_batch(seqs, quals, constraints=cons)
    want = res.pair_posteriors(x, 0.0)
    assert all(w[2].max() > 0.5 for w, c in zip(want, cons) if c is not None)
    want_t = res.train_eval(x)
    st = api.Engine(P1, PAR, W, 30, 1e-4, 0.1, 0, 0)
    st.set_option("max_resident", 2)
    st.load_batch(seqs, quals, constraints=cons)
    for sweep in range(2):          # (the second from the mask cache)
        got = st.pair_posteriors(x, 0.0)
        for k, (g, w) in enumerate(zip(got, want)):
            assert np.array_equal(g[0], w[0]) and np.array_equal(g[1], w[1]), (sweep, k)
            np.testing.assert_allclose(g[2], w[2], rtol=0, atol=1e-12, err_msg=str((sweep, k)))
            np.testing.assert_allclose(g[3], w[3], rtol=0, atol=1e-12, err_msg=str((sweep, k)))
    got_t = st.train_eval(x)
    assert got_t[3] == want_t[3] and abs(got_t[0] - want_t[0]) <= 1e-9 * max(1.0, abs(want_t[0]))
    np.testing.assert_allclose(got_t[1], want_t[1], **GR_TOL)
    np.testing.assert_array_equal(st.bpp_eff(), res.bpp_eff())


@pytest.mark.parametrize("lens,W", [(NARROW, 20), (WIDE, 50)], ids=["narrow", "wide"])
def test_an_all_free_load_is_a_plain_load(lens, W):
    seqs, quals = shape_batch(lens, 300)
    plain = api.Engine(P1, PAR, W, 30, 1e-4, 0.1, 0, 0)
    plain.load_batch(seqs, quals)
    eng = api.Engine(P1, PAR, W, 30, 1e-4, 0.1, 0, 0)
    eng.load_batch(seqs, quals, constraints=[None if k % 2 else "." * len(s) for k, s in enumerate(seqs)])
    x = perturbed(eng)
    for k in range(len(seqs)):
        assert np.array_equal(eng.pairs(k)[0], plain.pairs(k)[0]), k
    a, b = eng.scan(x), plain.scan(x)
    for k, (r, s) in enumerate(zip(a[0], b[0])):
        assert (r["Ys"], r["Ye"], r["rss"]) == (s["Ys"], s["Ye"], s["rss"]) and np.array_equal(r["psihat"], s["psihat"]), k
        assert r["exist_prob"] == pytest.approx(s["exist_prob"], rel=0, abs=1e-12)
    for k, (g, w) in enumerate(zip(eng.pair_posteriors(x, 0.0), plain.pair_posteriors(x, 0.0))):
        assert np.array_equal(g[0], w[0]) and np.array_equal(g[1], w[1]), k
        np.testing.assert_allclose(g[2], w[2], rtol=0, atol=1e-12)
        np.testing.assert_allclose(g[3], w[3], rtol=0, atol=1e-12)
    ta, tb = eng.train_eval(x), plain.train_eval(x)
    assert ta[3] == tb[3] and ta[2] == tb[2]
    np.testing.assert_allclose(ta[0], tb[0], rtol=0, atol=1e-12)
    np.testing.assert_allclose(ta[1], tb[1], rtol=0, atol=1e-12)


# ---- 2. the enumerated cases

@pytest.fixture(scope="module")
def enum_cases():
    return kc.enumerated_cases()


@pytest.mark.parametrize("opts", [(), (("fast", 0),), (("pipeline", 3),), (("poison", 1),)], ids=["default", "fast0", "pipeline3", "poison"])
def test_enumerated_cases_equal_the_enumeration(opts, enum_cases):
    U = 6
    for case, x, s, q, refs in enum_cases:
        pattern, L, flags, min_bpp = case
        eng = api.Engine(pattern, PAR, 50, 30, min_bpp, 0.1, flags, 0)
        for key, v in opts:
            eng.set_option(key, v)
        n = len(refs)
        eng.load_batch([s] * n, [q] * n, constraints=[c for c, _ in refs])
        fn, gr, eff, nsk = eng.train_eval(x)
        st = eng.seq_stats()
        assert np.all(np.isfinite(gr)) and (np.isfinite(fn) or nsk == n)
        pairs = eng.pair_posteriors(x, 0.0)
        ctx = eng.context_profiles(x)
        acc = eng.accessibility(x, U)
        nodes = eng.node_profiles(x)
        M = eng.n_node
        W = min(L, 50)
        for k, (c, e) in enumerate(refs):
            what = (case, c, opts)
            if not np.isfinite(e["lnZ"]):          # unsatisfiable: no parse, by the conventions of each call
                assert st[k, 4] == 1 and np.isneginf(st[k, 0]), what
                assert np.all(pairs[k][2] == 0.0) and np.array_equal(pairs[k][3], np.ones(L)), what
                assert np.array_equal(ctx[k], cc.exterior_only(L)), what
                assert np.array_equal(acc[k], ac.all_ones(L, U), equal_nan=True), what
                assert np.array_equal(nodes[k], nc.no_parse_profile(L, M)), what
                continue
            assert_log_close(st[k, 0], e["lnZ"], what=str(what))
            assert "node" in e, what          # (every enumerated case has at most node_check.MAX_ROWS rows)
            assert_log_close(st[k, 1], e["Zari"], what="Z(ari) %s" % (what,))
            assert_log_close(st[k, 2], e["Znasi"], what="Z(nasi) %s" % (what,))
            assert (st[k, 4] != 0) == (not np.isfinite(e["Zari"])), what          # skipped: no parse with the motif
            nc.assert_profile(nodes[k], e["node"], what=what, cols=range(M))
            P = pair_matrix(pairs[k], L, W)
            np.testing.assert_allclose(P, e["P"], rtol=1e-8, atol=1e-12, err_msg=str(what))
            np.testing.assert_allclose(pairs[k][3], e["unpaired"], rtol=1e-8, atol=1e-10, err_msg=str(what))
            cc.assert_profile(ctx[k], e["ctx"], what=what)
            ac.assert_access(acc[k], e["access"], what=what)


# ---- 3. / 4. conditioning and partition identities at the larger shapes, references from the oracle alone

BIG = [(47, 20, 147), (107, 50, 1107)]          # (L, max_span, synth seed)


def big_inputs(L, W, seed):
    """x, seq, qual, the oracle, its ln Z and its pair matrix"""
    (s,), (q,) = synth.synth_batch(1, L, seed=seed)
    x = perturbed(api.Engine(P1, PAR, W, 30, 1e-4, 0.1, 0, 0))
    o = cc.ctx_oracle(P1, W, 30, min_bpp=1e-4)
    o.set_params(x)
    P = oracle_pairs(o, s, q)
    assert P is not None
    return x, s, q, o, o.derivation_logz(s, q, None, None), P


def with_chars(L, chars):
    c = ["."] * L
    for p, ch in chars.items():
        c[p] = ch
    return "".join(c)


@pytest.mark.parametrize("L,W,seed", BIG, ids=["L47", "L107"])
def test_conditioning_identities(L, W, seed):
    """one sequence several times in one batch: a forced pair, an x window, a forced helix of three pairs; each ln Z_c - ln Z is
    the logarithm of the oracle's probability of the event"""
    x, s, q, o, lnZ, P = big_inputs(L, W, seed)
    i, d = np.unravel_index(np.argmax(P), P.shape)
    p_pair = P[i, d]
    U = 4
    acc = ac.table_access(o, s, q, x, U)[0]
    # the window of width U of largest probability among those that are not all but certain (such a one conditions on nothing)
    col = np.nan_to_num(acc[:, U - 1], nan=-1.0)
    col[col > 0.95] = -1.0
    w0 = int(np.argmax(col))
    p_win = acc[w0, U - 1]
    assert p_pair >= 0.05 and 0.05 <= p_win <= 0.95, (p_pair, p_win)
    strings = [None, with_chars(L, {i: "(", i + d - 1: ")"}), with_chars(L, {w0 + u: "x" for u in range(U)})]
    want = [0.0, np.log(p_pair), np.log(p_win)]
    # a helix of three directly stacked pairs around the likeliest pair that has one, by the oracle's helix reference
    from tests import helix_check as hc
    H = hc.table_helices(o, s, q, x, kmax=3)[:, :, 2]          # [a, b + 1]: the pairs (a, b), (a + 1, b - 1), (a + 2, b - 2) all form
    ha, hb1 = np.unravel_index(np.argmax(H), H.shape)
    p_hx, hb = H[ha, hb1], hb1 - 1
    assert p_hx >= 0.05, p_hx
    strings.append(with_chars(L, {ha: "(", ha + 1: "(", ha + 2: "(", hb: ")", hb - 1: ")", hb - 2: ")"}))
    want.append(np.log(p_hx))
    eng = api.Engine(P1, PAR, W, 30, 1e-4, 0.1, 0, 0)
    n = len(strings)
    eng.load_batch([s] * n, [q] * n, constraints=strings)
    eng.train_eval(x)
    st = eng.seq_stats()
    assert_log_close(st[0, 0], lnZ, what="free")
    for k in range(1, n):
        # (ln of a probability >= 0.05 from two ln Z of the project's 1e-9: the difference carries both errors)
        assert abs((st[k, 0] - st[0, 0]) - want[k]) <= 2e-9 * max(1.0, abs(lnZ)), (k, strings[k], st[k, 0] - st[0, 0], want[k])
    # the sampler under the same strings: every sample satisfies its string, and its logp is the weight of its derivation over
    # the constrained Z = oracle Z times the reference probability of the event.  Bound: sample_check.logp_atol on the two
    # log partition functions, plus 1e-8 for the logarithm of a reference probability that holds to the project's rtol 1e-8
    smp = eng.sample_structures(x, 8, seed=11)
    for k in range(1, n):
        rss, nodes, logp, status = smp[k]
        assert status == eng.SAMPLED, (k, status)
        for t in range(len(rss)):
            db = kc.letters_to_db(rss[t])
            assert kc.satisfies(db, strings[k]), (k, t, db)
            ref = o.derivation_logz(s, q, db, nodes[t]) - (lnZ + want[k])
            assert abs(logp[t] - ref) <= logp_atol(lnZ) + 1e-8, (k, t, logp[t], ref)


@pytest.mark.parametrize("L,W,seed", BIG, ids=["L47", "L107"])
def test_partition_identity_of_the_outside_based_products(L, W, seed):
    """X_free = a X_x + (1 - a) X_| for x and | on one base, a = the oracle's unpaired probability of that base"""
    x, s, q, o, lnZ, P = big_inputs(L, W, seed)
    u = unpaired_of(P, L)
    p = int(np.argmin(np.abs(u - 0.5)))
    a = u[p]
    assert 0.05 <= a <= 0.95, a
    eng = api.Engine(P1, PAR, W, 30, 1e-4, 0.1, 0, 0)
    eng.load_batch([s] * 3, [q] * 3, constraints=[None, with_chars(L, {p: "x"}), with_chars(L, {p: "|"})])

    def mix(X):
        return a * X[1] + (1.0 - a) * X[2]

    pairs = eng.pair_posteriors(x, 0.0)
    Pm = [pair_matrix(e, L, W) for e in pairs]
    np.testing.assert_allclose(Pm[0], mix(Pm), rtol=1e-8, atol=3e-12, err_msg="pairs")
    np.testing.assert_allclose(Pm[0], P, rtol=1e-8, atol=1e-12, err_msg="pairs of the free copy against the oracle")
    un = [e[3] for e in pairs]
    np.testing.assert_allclose(un[0], mix(un), rtol=1e-8, atol=3e-10, err_msg="unpaired")
    assert abs(un[1][p] - 1.0) <= 1e-10 and abs(un[2][p]) <= 1e-10
    for name, X in (("context", eng.context_profiles(x)), ("node", eng.node_profiles(x)), ("accessibility", eng.accessibility(x, 8)),
                    ("joint counts", list(eng.joint_profiles(x))), ("stem counts", list(eng.stem_profiles(x)))):
        got, ref = np.asarray(X[0]), mix([np.asarray(v) for v in X])
        assert np.array_equal(np.isnan(got), np.isnan(ref)), name
        np.testing.assert_allclose(got, ref, rtol=1e-8, atol=3e-10, err_msg=name)
    # helix and loop posteriors (their checks' rtol 1e-8, atol 1e-10, the latter times 3): the lists at min_prob 0 hold every kept
    # cell of each copy's own mask, so they are compared as dense arrays, zero where a copy has no entry
    K = 8
    hx = [hc.dense_from_list(L, K, lst) for lst in eng.helix_posteriors(x, 0.0, 1, K)]
    assert hx[0][:, :, 2].max() >= 0.05
    np.testing.assert_allclose(hx[0], mix(hx), rtol=1e-8, atol=3e-10, err_msg="helix")
    closing, two, counts = eng.loop_posteriors(x, 0.0)
    dense = [lc.dense_from_closing(L, lst) for lst in closing]
    cols = [d[0] for d in dense]
    for t, letter in enumerate("HSBIM"):
        assert cols[0][:, :, t].max() > 0 or letter == "M", letter
    np.testing.assert_allclose(cols[0], mix(cols), rtol=1e-8, atol=3e-10, err_msg="loop columns")
    np.testing.assert_allclose(dense[0][1], mix([d[1] for d in dense]), rtol=1e-8, atol=3e-10, err_msg="pair column of the closing list")
    np.testing.assert_allclose(counts[0], mix(list(counts)), rtol=1e-8, atol=3e-10, err_msg="loop counts")
    td = [lc.two_dict(lst) for lst in two]
    keys = sorted(set(td[0]) | set(td[1]) | set(td[2]))
    tv = [np.array([d.get(key, 0.0) for key in keys]) for d in td]
    assert len(keys) > 0 and tv[0].max() >= 1e-3
    np.testing.assert_allclose(tv[0], mix(tv), rtol=1e-8, atol=3e-10, err_msg="two-loops")


# ---- 5. the sampler and the CYK structure

@pytest.mark.parametrize("lens,W", [(NARROW, 20), (WIDE[:5], 50)], ids=["narrow", "wide"])
def test_samples_and_the_scan_structure_satisfy_their_strings(lens, W):
    """the strings are drawn from the CYK structure of the free fold, which satisfies them: a sequence whose free scan has a parse
    keeps one, and every structure that comes out satisfies its string"""
    seqs, quals = shape_batch(lens, 300)
    cons, x = structure_strings(seqs, quals, W, 70)
    eng = api.Engine(P1, PAR, W, 30, 1e-4, 0.1, 0, 0)
    eng.load_batch(seqs, quals, constraints=cons)
    recs, _ = eng.scan(x)
    smp = eng.sample_structures(x, 20, seed=5)
    for k, c in enumerate(cons):
        if c is None:
            continue
        rss, _, logp, status = smp[k]
        assert status == eng.SAMPLED, (k, c, status)
        for t in rss:
            assert kc.satisfies(kc.letters_to_db(t), c), (k, c, t)
        assert np.all(np.isfinite(logp)) and np.all(logp <= 1e-9)
        assert recs[k]["rss"].strip() and kc.satisfies(kc.letters_to_db(recs[k]["rss"]), c), (k, c, recs[k]["rss"])
        for p, ch in enumerate(c):          # no L / R letter on x, L at a ( or <, R at a ) or >
            t = recs[k]["rss"][p]
            assert (ch != "x" or t not in "LR") and (ch not in "(<" or t == "L") and (ch not in ")>" or t == "R"), (k, p, ch, t)


# ---- 6. a whole structure

def whole_inputs(which):
    """pattern, W, x, seq, qual, oracle of a whole-structure case: the larger shapes, and the pattern of 64 interval states of
    tests/large_automata.py on its planted sequence of 70 bases"""
    if which == "S64":
        pattern, W = la.PATTERN[64], 50
        s, q = la.planted(70, 6470)
    else:
        L, W, seed = BIG[1] if which == "L107" else BIG[0]
        pattern = P1
        (s,), (q,) = synth.synth_batch(1, L, seed=seed)
    x = perturbed(api.Engine(pattern, PAR, W, 30, 1e-4, 0.1, 0, 0))
    o = cc.ctx_oracle(pattern, W, 30, min_bpp=1e-4)
    o.set_params(x)
    return pattern, W, x, s, q, o


@pytest.mark.parametrize("which", ["L47", "L107", "S64"])
def test_a_whole_structure_given_back_as_the_string(which):
    pattern, W, x, s, q, o = whole_inputs(which)
    L = len(s)
    free = api.Engine(pattern, PAR, W, 30, 1e-4, 0.1, 0, 0)
    if which == "S64":
        assert free.n_state == 64
    free.load_batch([s], [q])
    db = free.mea_structures(x, 1.0)[0][0]
    assert "(" in db
    cons = db.replace(".", "x")
    eng = api.Engine(pattern, PAR, W, 30, 1e-4, 0.1, 0, 0)
    eng.load_batch([s], [q], constraints=[cons])
    eng.train_eval(x)
    assert_log_close(eng.seq_stats()[0, 0], o.derivation_logz(s, q, db, None), what="ln Z of one structure")
    ii, jj, pp, unp = eng.pair_posteriors(x, 0.0)[0]
    want = sorted((a, b + 1) for a, b in kc.forced_pairs(cons))
    assert sorted(zip(ii.tolist(), jj.tolist())) == want
    np.testing.assert_allclose(pp, 1.0, rtol=0, atol=1e-10)
    np.testing.assert_allclose(unp, [1.0 if c == "." else 0.0 for c in db], rtol=0, atol=1e-10)
    assert eng.mea_structures(x, 1.0)[0][0] == db
    assert eng.scan(x)[0][0]["rss"].replace("L", "(").replace("R", ")").translate(str.maketrans("OHBIM", ".....")) == db
    # the node profile against the table reference on an oracle made with DBG_FIX_RSS (on the CPU that reference equals the
    # enumeration over node rows for one structure of a tiny case: tests/test_constraint_cpu.py)
    of = cc.ctx_oracle(pattern, W, 30, min_bpp=1e-4, flags=po.DBG_FIX_RSS)
    ref = nc.table_profile(kc.FixedOracle(of, db, W), s, q, x)
    assert ref is not None
    nc.assert_profile(eng.node_profiles(x)[0], ref, what=which, cols=range(eng.n_node))


# ---- 7. the train switches

@pytest.mark.parametrize("lens,W", [(NARROW, 20), (WIDE, 50)], ids=["narrow", "wide"])
def test_train_switches_agree_on_a_constrained_batch(lens, W):
    """(strings drawn from the CYK structures of the free fold: every constrained sequence keeps a parse with the motif)"""
    seqs, quals = shape_batch(lens, 300)
    cons, x = structure_strings(seqs, quals, W, 90)
    base = api.Engine(P1, PAR, W, 30, 1e-4, 0.1, 0, 0)
    base.load_batch(seqs, quals, constraints=cons)
    fn0, gr0, eff0, nsk0 = base.train_eval(x)
    st0, c0 = base.seq_stats(), base.seq_counts()
    assert all(st0[k, 4] == 0 for k, c in enumerate(cons) if c is not None)
    for key in SWITCHES:
        eng = api.Engine(P1, PAR, W, 30, 1e-4, 0.1, 0, 0)
        eng.set_option(key, 0)
        eng.load_batch(seqs, quals, constraints=cons)
        fn, gr, eff, nsk = eng.train_eval(x)
        assert nsk == nsk0 and eff == eff0, key
        assert abs(fn - fn0) <= 1e-9 * max(1.0, abs(fn0)), (key, fn, fn0)
        np.testing.assert_allclose(gr, gr0, err_msg=key, **GR_TOL)
        assert_log_close(eng.seq_stats()[:, :3], st0[:, :3], what=key)
        c = eng.seq_counts()
        for name in c0:
            np.testing.assert_allclose(c[name], c0[name], rtol=ROW_RTOL, atol=ROW_ATOL, err_msg="%s %s" % (key, name))


# ---- 8. refusals

def test_refused_loads_leave_the_handle_usable():
    seqs, quals = shape_batch((33, 21), 300)
    eng = api.Engine(P1, PAR, 20, 30, 1e-4, 0.1, 0, 0)
    s = seqs[0]
    i, j = next((i, j) for i in range(33) for j in range(i + 4, min(33, i + 20)) if (int(s[i]), int(s[j])) not in kc.PAIRING)
    bad = [with_chars(33, {3: "("}), with_chars(33, {9: ")"}), with_chars(33, {4: "y"}), with_chars(33, {i: "(", j: ")"})]
    msgs = ["unbalanced", "unbalanced", "unknown character 'y' at position 4", "bases %d and %d" % (i, j)]
    for c, m in zip(bad, msgs):
        with pytest.raises(api.ElemdpError) as e:
            eng.load_batch(seqs, quals, constraints=[c, None])
        assert e.value.code == -1 and m in str(e.value) and "sequence 0" in str(e.value), (c, str(e.value))
        with pytest.raises(api.ElemdpError) as e:          # (a refused load leaves no batch)
            eng.train_eval(perturbed(eng))
        assert e.value.code == -4
    eng.load_batch(seqs, quals, constraints=[None, "x" * 21])
    fn, gr, _, _ = eng.train_eval(perturbed(eng))
    assert np.isfinite(fn) and np.all(np.isfinite(gr))
    for pattern, flags, fix in ((P1, api.DBG_FIX_RSS, ["." * 33, "." * 21]), ("..*..", api.NO_RSS, None)):
        e2 = api.Engine(pattern, PAR, 20, 30, 1e-4, 0.1, flags, 0)
        with pytest.raises(api.ElemdpError) as e:
            e2.load_batch(seqs, quals, constraints=[None, None])
        assert e.value.code == -1
        e2.load_batch(seqs, quals, fix_rss=fix)
        e2.train_eval(perturbed(e2))


# ---- 9. the command line's scan under constraints, in chunks and over two ranks

NUMBER = re.compile(r"-?\d+(?:\.\d+)?(?:e[-+]?\d+)?")


def assert_same_text(got, want):
    """the same text but for the last printed digit of a number (six digits are printed; a probability that is 0 in one run may
    be 1e-17 in another, whose groups sum in another order)"""
    assert NUMBER.sub("#", got) == NUMBER.sub("#", want)
    g, w = [float(v) for v in NUMBER.findall(got)], [float(v) for v in NUMBER.findall(want)]
    np.testing.assert_allclose(g, w, rtol=1e-5, atol=1e-9)


def test_scan_records_in_chunks_and_ranks_equal_one_constrained_load(tmp_path):
    seqs, quals = shape_batch(WIDE[:7], 300)
    cons, x = structure_strings(seqs, quals, 50, 70)
    cons[1] = None          # (a record the file does not name)
    recs = [("@r%d" % k, s, q) for k, (s, q) in enumerate(zip(seqs, quals))]
    m = dict(x=x)
    eng = api.Engine(P1, PAR, 50, 30, 1e-4, 0.1, 0, 0)
    nodes = eng.describe()["node"]
    eng.load_batch(seqs, quals, constraints=cons)
    res, _ = eng.scan(x)
    prs = eng.pair_posteriors(x, 1e-3)
    want1 = "".join(io.scan_record(rid, s, r, nodes) for (rid, s, _), r in zip(recs, res))
    wantp = "# constraints: c.txt\n" + "".join(io.pair_record(rid, len(s), (ii, jj, pp), unp) for (rid, s, _), (ii, jj, pp, unp) in zip(recs, prs))
    for world, chunk in ((1, 2), (2, 3), (1, 100)):
        out1, outp = str(tmp_path / ("scan%d%d.raw" % (world, chunk))), str(tmp_path / ("pairs%d%d.txt" % (world, chunk)))
        for rank in reversed(range(world)):
            cli._scan_records(eng, m, recs, out1, chunk, rank, world, lambda: None, out_pairs=outp, constraints=cons, constraints_path="c.txt")
        assert_same_text(open(out1).read(), want1)
        assert_same_text(open(outp).read(), wantp)
    for k, c in enumerate(cons):          # (and the strings reached their own records: every printed structure satisfies its string)
        if c is not None:
            assert kc.satisfies(kc.letters_to_db(res[k]["rss"]), c), k
