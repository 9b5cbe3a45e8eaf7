"""Scan posteriors in one world on the GPU: every call that honours option world against the references of
tests/world_check.py -- the enumeration on the tiny cases, the oracle's tables at the lengths around W = 20 and on a batch at W = 50
--, the mixture identity on the engine's own outputs, the agreement with conditional_pairs, empty worlds under poisoned table
slots, both forms in one call, groupings and a streamed batch, the mixture after a world call, the sampler, the sites, the command
line and the refusals."""
import ctypes as C

import numpy as np
import pytest

from rnaelem_amd import api, cli, io
from tests import cond_check as cd
from tests import ctx_check as cc
from tests import node_check as nc
from tests import node_mea_check as mc
from tests import world_check as wc
from tests.mea_mirror import mea_fold, pair_matrix
from tests.test_cond_cpu import motif_heavy
from tests.test_ctx_cpu import CASES
from tests.test_ctx_gpu import pool_map
from tests.test_pair_posterior_gpu import perturbed
from tests.test_pair_shapes_gpu import P1, PAR, batch
from tests.test_world_cpu import WORLD_METHODS, references
from tests.util import gpath

pytestmark = pytest.mark.gpu

P3 = "(.*)"
WORLDS = wc.WORLDS
_REFS = {}


def cached(key, compute):
    if key not in _REFS:
        _REFS[key] = compute()
    return _REFS[key]


def engine_with(pattern, W, opts=()):
    eng = api.Engine(pattern, PAR, W, 30, 1e-4, 0.1, 0, 0)
    for k, v in opts:
        eng.set_option(k, v)
    return eng


def table_refs(pattern, W, x, seqs, quals, products=wc.ALL_PRODUCTS):
    """world_check.table_worlds of every sequence over a thread pool"""
    xn = cd.none_params(x, cc.ctx_oracle(pattern, W, 30).hmm())
    order = sorted(range(len(seqs)), key=lambda k: -len(seqs[k]))
    got = pool_map(lambda: (cc.ctx_oracle(pattern, W, 30), cc.ctx_oracle(pattern, W, 30)),
                   lambda oo, k: wc.table_worlds(oo[0], oo[1], x, xn, seqs[k], quals[k], products), order)
    out = [None] * len(seqs)
    for k, v in zip(order, got):
        out[k] = v
    return out


def check_empty(got, L, W, M, K, what=""):
    """the dense products of a sequence whose world is empty: what every call returns for a sequence without a parse, exactly"""
    want = wc.empty_world(L, W, M, K)
    for p, v in want.items():
        if p in got:
            assert np.array_equal(got[p], v, equal_nan=True), (what, p)
    for p in ("loop_counts", "stem_counts"):
        if p in got:
            assert not np.any(got[p]), (what, p)
    if "two" in got:
        assert got["two"] == {}, what
    if "joint_counts" in got:
        assert got["joint_counts"].sum() == L and got["joint_counts"][0, 0].sum() == L, (what, "joint counts")


def check_worlds(eng, x, seqs, refs, products=wc.ALL_PRODUCTS, what=""):
    """both worlds of every product of the resident batch against the table references: reference 1 for the world without the
    motif, reference 2 for the world with it, the conventions for an empty world.  Returns {world: products per sequence}."""
    M, K = eng.n_node, len(eng.stem_slots())
    slots = eng.stem_slots()
    out = {}
    for w in WORLDS:
        out[w] = got = wc.engine_products(eng, x, w, seqs, products)
        for k, (g, ref) in enumerate(zip(got, refs)):
            L, W = len(seqs[k]), min(len(seqs[k]), eng.max_span)
            if not np.isfinite(ref["Zari" if w == "motif" else "Znasi"]):
                check_empty(g, L, W, M, K, what=(what, w, k, L))
                continue
            r = dict(ref)
            r[w] = wc.by_slots(ref[w], slots)
            wc.assert_world(g, r, w, what=(what, k, L))
    return out


# ---- 1. the tiny cases against the enumeration

@pytest.mark.parametrize("case", CASES, ids=lambda c: "%s-%d-%g" % c)
@pytest.mark.parametrize("opts", [(), (("fast", 0),), (("pipeline", 3),)], ids=["default", "fast0", "pipeline3"])
def test_tiny_cases_equal_the_enumeration_in_both_worlds(opts, case):
    pattern, flags, min_bpp = case
    x, seqs, quals, enum, tab = references(case)
    eng = api.Engine(pattern, PAR, 50, 30, min_bpp, 0.1, flags, 0)
    for k, v in opts:
        eng.set_option(k, v)
    eng.load_batch(seqs, quals)
    got = {w: wc.engine_products(eng, x, w, seqs, ("pairs", "context", "nodes", "access", "loops")) for w in WORLDS}
    if not any(k == "pipeline" for k, _ in opts):
        assert eng.last_timing()[2] == 0      # (no world is empty here: no sequence handed on)
    differ = 0.0
    for k, e in enumerate(enum):
        for w in WORLDS:
            wc.assert_enumerated(got[w][k], e, w, what=(opts, case, k, w))
        differ = max(differ, np.abs(got["motif"][k]["context"] - got["none"][k]["context"]).max())
    assert differ > 0.01, differ      # (the worlds differ: a swap, or the mixture in place of a world, cannot pass)


# ---- 2. larger shapes against the tables of both worlds

W20_LENS = (1, 5, 19, 20, 21, 47)
W50_LENS = (107, 3, 50, 51, 64, 88, 12, 33, 100)


def shape_case(pattern, W, lens):
    """(seqs, quals, x with the pattern rows raised by 3, table references of both worlds)"""
    def compute():
        seqs, quals = batch(lens, seed=31 + W, neg_every=0)
        o = cc.ctx_oracle(pattern, W, 30)
        x = motif_heavy(perturbed(engine_with(pattern, W)), o.hmm())
        return seqs, quals, x, table_refs(pattern, W, x, seqs, quals)
    return cached(("shape", pattern, W, lens), compute)


@pytest.mark.parametrize("pattern,W,lens", [(P1, 20, W20_LENS), (P3, 20, W20_LENS), (P1, 50, W50_LENS), (P3, 50, W50_LENS)],
                         ids=["P1-W20", "P3-W20", "P1-W50", "P3-W50"])
@pytest.mark.parametrize("opts", [(), (("pipeline", 3),)], ids=["lin", "log"])
def test_shapes_against_the_tables_of_both_worlds(pattern, W, lens, opts):
    seqs, quals, x, refs = shape_case(pattern, W, lens)
    # reference 2 holds for the whole batch: every sequence has e >= E_MIN, or no parse with the motif at all (too short for the
    # pattern: an empty world, held to its conventions exactly)
    assert all(r["e"] >= wc.E_MIN or not np.isfinite(r["Zari"]) for r in refs), [r["e"] for r in refs]
    assert all(np.isfinite(r["Znasi"]) for r in refs) and sum(np.isfinite(r["Zari"]) for r in refs) >= len(refs) - 2
    eng = engine_with(pattern, W, opts)
    eng.load_batch(seqs, quals)
    check_worlds(eng, x, seqs, refs, what=(pattern, W, opts))


# ---- 3. the mixture identity on the engine's own outputs, 4. the agreement with conditional_pairs

@pytest.fixture(scope="module")
def ordinary():
    """the ordinary model (no raised rows) on a batch at W = 50: the engine, x, the three worlds of every product, the conditional
    call's records"""
    seqs, quals = batch((30, 61, 100, 5, 47), seed=12, neg_every=0)
    eng = engine_with(P1, 50)
    eng.load_batch(seqs, quals)
    x = perturbed(eng)
    got = {w: wc.engine_products(eng, x, w, seqs) for w in ("mixed",) + WORLDS}
    assert eng.world == "mixed"
    con = eng.conditional_pairs(x, 0.0, 1.0)
    return eng, x, seqs, quals, got, con


def test_the_worlds_mix_into_the_mixture(ordinary):
    """e X_motif + (1 - e) X_none = X_mixed for every product of the eleven calls that is an expectation, whatever e is"""
    eng, x, seqs, quals, got, con = ordinary
    es = []
    for k in range(len(seqs)):
        e = con[k]["exist_prob"]
        es.append(e)
        wc.assert_mixture(got["mixed"][k], got["motif"][k], got["none"][k], e, what=(k, len(seqs[k]), e))
    assert min(es) == 0.0 and 0.0 < sorted(es)[1] and max(es) < 1.0, es      # (L = 5 has no parse with the motif)
    assert max(np.abs(got["motif"][k]["nodes"] - got["none"][k]["nodes"]).max() for k in range(len(seqs))) > 0.5


def test_pair_posteriors_in_a_world_are_the_conditional_call(ordinary):
    """P_motif and P_none of conditional_pairs at 1e-12 (two calls do not give the same bits: DESIGN.md section 24), and the MEA
    structure of each world through the mirror on the call's own P"""
    eng, x, seqs, quals, got, con = ordinary
    for w in WORLDS:
        structs, scores, pairs = eng.mea_structures(x, 1.0, 0.0, world=w)
        for k, rec in enumerate(con):
            L, W = len(seqs[k]), min(len(seqs[k]), eng.max_span)
            Pc, listed = pair_matrix(L, W, rec["i"], rec["j"], rec["p_" + w])
            np.testing.assert_allclose(got[w][k]["pairs"], Pc, rtol=0, atol=1e-12, err_msg=str((w, k)))
            np.testing.assert_allclose(got[w][k]["unpaired"], rec["unpaired_" + w], rtol=0, atol=1e-12, err_msg=str((w, k)))
            ii, jj, pp, unp = pairs[k]
            assert np.array_equal(ii, rec["i"]) and np.array_equal(jj, rec["j"]), (w, k)
            P, kept = pair_matrix(L, W, ii, jj, pp)
            assert structs[k] == mea_fold(P, kept, unp, 1.0)[0], (w, k)
            if np.array_equal(P, Pc) and np.array_equal(unp, rec["unpaired_" + w]):
                assert structs[k] == rec["structure_" + w], (w, k)
    assert any(r["structure_motif"] != r["structure_none"] for r in con)


# ---- 5. empty worlds

def every_call(eng, x, seqs, world):
    """every call that honours the option, in one world: the dense products, the MEA structures, the sites and the samples"""
    got = wc.engine_products(eng, x, world, seqs)
    structs, scores, _ = eng.mea_structures(x, 1.0, world=world)
    sites = eng.mea_alignments(x, 1.0, 2, world=world)
    samples = eng.sample_structures(x, 6, seed=5, world=world)
    db = ["." * len(s) for s in seqs]
    stems = eng.helix_posteriors(x, np.inf, 1, 4, structures=db, world=world)[1]
    loops = eng.loop_posteriors(x, np.inf, structures=db, world=world)[3]
    return got, structs, sites, samples, stems, loops


def check_empty_calls(eng, k, L, calls, what=""):
    got, structs, sites, samples, stems, loops = calls
    check_empty(got[k], L, min(L, eng.max_span), eng.n_node, len(eng.stem_slots()), what=what)
    assert structs[k] == "." * L, what
    assert len(sites[k]["start"]) == 0 and sites[k]["rows"].shape == (0, L), what
    rss, nodes, logp, status = samples[k]
    assert status == eng.NO_PARSE and np.all(np.isnan(logp)) and not nodes.any(), what
    assert len(stems[k][0]) == 0 and len(loops[k][0]) == 0, what


@pytest.mark.parametrize("opts", [(("poison", 1),), (("poison", 1), ("pipeline", 3))], ids=["lin", "log"])
def test_a_sequence_shorter_than_the_pattern_has_an_empty_motif_world(opts):
    seqs, quals = batch((5, 40, 3, 26), seed=8, neg_every=0)
    eng = engine_with(P1, 50, opts)
    eng.load_batch(seqs, quals)
    x = perturbed(eng)
    refs = table_refs(P1, 50, x, seqs, quals, ("pairs", "context", "nodes"))
    assert [np.isfinite(r["Zari"]) for r in refs] == [False, True, False, True] and all(np.isfinite(r["Znasi"]) for r in refs)
    calls = every_call(eng, x, seqs, "motif")
    for k in (0, 2):
        check_empty_calls(eng, k, len(seqs[k]), calls, what=(opts, k))
    for k in (1, 3):      # (the neighbours in the same group keep their world)
        assert calls[0][k]["pairs"].max() > 0.1 and np.all(np.isfinite(calls[0][k]["context"])), k
        assert calls[3][k][3] == eng.SAMPLED
    # the world without the motif is whole for every sequence, and the handle is usable afterwards
    check_worlds(eng, x, seqs, refs, ("pairs", "context", "nodes"), what=opts)
    recs, _ = eng.scan(x)
    assert len(recs) == 4 and eng.world == "mixed"


@pytest.mark.parametrize("opts", [(("poison", 1),), (("poison", 1), ("pipeline", 3))], ids=["lin", "log"])
def test_without_the_background_row_the_world_without_the_motif_is_empty(opts):
    """theta row 0 at -inf: no parse without the motif, and the world with it is the mixture (hairpins that the motif covers from
    end to end: a base outside the motif would be emitted with row 0)"""
    seqs = [np.array(["NACGU".index(c) for c in s], dtype=np.uint8) for s in ("GGAAACC", "GGGAAACCC", "GGGAAAACCC", "GCGAAAGC", "GGGGAAAACCCC")]
    quals = [np.full(len(s) + 1, 10, dtype=np.uint8) for s in seqs]
    eng = engine_with(P1, 50, opts)
    eng.load_batch(seqs, quals)
    x = perturbed(eng)
    x[:eng.describe()["theta_sizes"][0]] = -np.inf
    o = cc.ctx_oracle(P1, 50, 30)
    o.set_params(x)
    for s, q in zip(seqs, quals):
        t = o.train_seq(s, q)
        assert not np.isfinite(t["Znasi"]) and np.isfinite(t["Zari"]) and t["Zari"] == t["Zo"]
    calls = every_call(eng, x, seqs, "none")
    for k in range(len(seqs)):
        check_empty_calls(eng, k, len(seqs[k]), calls, what=(opts, k))
    mixed, motif = wc.engine_products(eng, x, "mixed", seqs), wc.engine_products(eng, x, "motif", seqs)
    for k in range(len(seqs)):
        wc.assert_mixture(mixed[k], motif[k], motif[k], 1.0, what=k)
        assert np.isfinite(motif[k]["context"]).all() and motif[k]["pairs"].max() > 0.1
    assert eng.sample_structures(x, 4, seed=1, world="motif")[0][3] == eng.SAMPLED


# ---- 6. both forms in one call

def test_sequences_out_of_the_double_range_take_the_log_space_form():
    """lambda = 40: the long sequences leave the double range of the scaled-linear tables and go through the fused scan kernel, the
    short ones stay on the scaled-linear path -- both forms in one call, and they agree with the conditional call and the mixture"""
    recs = io.read_fastq(gpath("syn_L150_n8.fq"))
    short_s, short_q = batch((4, 9, 16, 24), seed=40, neg_every=0)
    seqs = short_s[:2] + [s for _, s, _ in recs][:3] + short_s[2:]
    quals = short_q[:2] + [q for _, _, q in recs][:3] + short_q[2:]
    eng = engine_with(P1, 50, (("group", 2),))
    eng.load_batch(seqs, quals)
    x = eng.initial_params(40.0)
    prods = ("pairs", "context", "access", "loops")
    refs = table_refs(P1, 50, x, seqs, quals, ("pairs", "context"))
    got = {}
    for w in ("mixed",) + WORLDS:
        got[w] = wc.engine_products(eng, x, w, seqs, prods)
        n_log = eng.last_timing()[2]
        assert 3 <= n_log < len(seqs), (w, n_log)
    con = eng.conditional_pairs(x, 0.0)
    for k in range(len(seqs)):
        L, W = len(seqs[k]), min(len(seqs[k]), 50)
        # (the loop counts of a sequence in the log-space form are sums of probabilities that carry 1e-13 each at this ln Z)
        wc.assert_mixture(got["mixed"][k], got["motif"][k], got["none"][k], con[k]["exist_prob"], what=k, count_rtol=1e-12)
        for w in WORLDS:
            np.testing.assert_allclose(got[w][k]["pairs"], pair_matrix(L, W, con[k]["i"], con[k]["j"], con[k]["p_" + w])[0], rtol=0, atol=1e-12)
        if np.isfinite(refs[k]["Znasi"]):
            wc.assert_world(got["none"][k], refs[k], "none", ("pairs", "unpaired", "context"), what=k)


# ---- 7. groupings and a streamed batch

def same_products(a, b, tol):
    assert len(a) == len(b)
    for k, (r, s) in enumerate(zip(a, b)):
        assert set(r) == set(s), k
        for key in r:
            if key == "two":
                assert set(r[key]) == set(s[key]), (k, key)
                np.testing.assert_allclose([r[key][t] for t in sorted(r[key])], [s[key][t] for t in sorted(s[key])], **tol)
            else:
                np.testing.assert_allclose(r[key], s[key], equal_nan=True, err_msg=str((k, key)), **tol)


@pytest.fixture(scope="module")
def grouped():
    lens = [int(v) for v in np.linspace(5, 140, 7)][::-1]
    lens[1], lens[4] = lens[4], lens[1]
    seqs, quals = batch(lens, seed=5, neg_every=0)
    base = engine_with(P1, 50)
    base.load_batch(seqs, quals)
    x = perturbed(base)
    return seqs, quals, x, {w: wc.engine_products(base, x, w, seqs) for w in WORLDS}


@pytest.mark.parametrize("opts", [(("group", 1),), (("group", 3),), (("max_resident", 2),)], ids=lambda o: "%s-%d" % o[0])
def test_groupings_and_a_streamed_batch_give_the_same_products(opts, grouped):
    """(two runs agree to rounding: the sweeps gather through LDS atomics.)  The streamed batch also shows that the option reaches
    the inner engines, that setting it keeps the cached masks and that it takes one entry of the option record however often a call
    sets it"""
    seqs, quals, x, want = grouped
    eng = engine_with(P1, 50, opts)
    eng.load_batch(seqs, quals)
    n0 = eng.options_logged()
    for w in WORLDS:
        same_products(wc.engine_products(eng, x, w, seqs), want[w], dict(rtol=1e-10, atol=1e-14))
    assert eng.options_logged() == n0 + 1 and eng.world == "mixed"


# ---- 8. the mixture after a world call; scan and the conditional call ignore the option

def test_a_world_call_leaves_the_mixture_and_the_other_calls_alone():
    seqs, quals = batch((30, 61, 100), seed=12, neg_every=0)
    x = perturbed(engine_with(P1, 50))
    tol = dict(rtol=0, atol=1e-12)      # the floats of a world-0 call after a world call against a fresh handle's
    # scan and conditional_pairs under the option against the same calls without it: two runs of one call, which agree to rounding
    # only (the sum passes gather through LDS atomics).  The bound is the one test_cond_gpu.test_other_calls_are_untouched holds two
    # runs of these calls to -- the relative term is for the scan's log posteriors and E[N], which are not bounded by 1
    runs = dict(rtol=1e-10, atol=1e-12)

    def mixture(eng):
        return (wc.engine_products(eng, x, "mixed", seqs), eng.mea_structures(x, 1.0)[0], eng.mea_alignments(x, 1.0, 2),
                eng.sample_structures(x, 10, seed=3))

    fresh = engine_with(P1, 50)
    fresh.load_batch(seqs, quals)
    want = mixture(fresh)
    scan0, en0 = fresh.scan(x)
    con0 = fresh.conditional_pairs(x, 0.0, 1.0)
    eng = engine_with(P1, 50)
    eng.load_batch(seqs, quals)
    wc.engine_products(eng, x, "motif", seqs)
    eng.sample_structures(x, 10, seed=3, world="motif")
    got = mixture(eng)
    same_products(got[0], want[0], tol)
    assert got[1] == want[1]
    for a, b in zip(got[2], want[2]):
        assert np.array_equal(a["rows"], b["rows"]) and np.array_equal(a["start"], b["start"]) and np.array_equal(a["end"], b["end"])
    for (ra, na, la, sa), (rb, nb, lb, sb) in zip(got[3], want[3]):
        assert list(ra) == list(rb) and np.array_equal(na, nb) and sa == sb
        np.testing.assert_allclose(la, lb, **tol)
    # scan and conditional_pairs under option world 1 and 2 are what they are under 0
    for v in (1, 2):
        eng.set_option("world", v)
        scan1, en1 = eng.scan(x)
        for a, b in zip(scan0, scan1):
            assert a["rss"] == b["rss"] and (a["Ys"], a["Ye"]) == (b["Ys"], b["Ye"]) and np.array_equal(a["psihat"], b["psihat"])
            np.testing.assert_allclose(b["exist_prob"], a["exist_prob"], **runs)
            for key in ("start", "inner", "end"):
                np.testing.assert_allclose(b[key], a[key], **runs)
        np.testing.assert_allclose(en1, en0, **runs)
        cd.same_records(eng.conditional_pairs(x, 0.0, 1.0), con0, **runs)
    eng.set_option("world", 0)


# ---- 9. the sampler

def test_the_sampler_draws_in_one_world():
    """L = 20 and 47 (and 5: an empty motif world) at W = 20, 50 samples: the draws of the CPU driver given the same world, every
    logp against the weight of the derivation relative to Z_w, node 0 everywhere without the motif and an inner node with it"""
    seqs, quals = batch((20, 47, 5), seed=77, neg_every=0)
    eng = engine_with(P1, 20)
    eng.load_batch(seqs, quals)
    o = cc.ctx_oracle(P1, 20, 30)
    x = motif_heavy(perturbed(eng), o.hmm(), by=1.0)
    o.set_params(x)
    drv = wc.WorldDriver(P1, PAR, 20, 30, 1e-4, 0.1, 0)
    for opts in ((), (("pipeline", 3),)):
        for k, v in opts:
            eng.set_option(k, v)
        for w, world in ((1, "motif"), (2, "none")):
            res = eng.sample_structures(x, 50, seed=11, index_base=3, world=world)
            same = total = 0
            for k, (s, q) in enumerate(zip(seqs, quals)):
                n_distinct = wc.check_samples(o, s, q, res[k], world, eng.n_node, what=(opts, world, k))
                assert n_distinct > 3 or len(s) < 20, (opts, world, k, n_distinct)      # (L = 5 has one structure: all exterior)
                if not opts:      # (the driver has the scaled-linear form)
                    want = drv.sample(x, s, q, 50, 11, 3 + k, w)
                    assert want[3] == res[k][3]
                    same += sum(a == b and np.array_equal(c, d) for a, b, c, d in zip(res[k][0], want[0], res[k][1], want[1]))
                    total += 50
            assert same >= 0.999 * total, (world, same, total)
    eng.set_option("pipeline", 4)


# ---- 10. the sites

def test_sites_of_the_motif_world_follow_its_node_profile():
    seqs, quals, x, refs = shape_case(P1, 50, W50_LENS)
    eng = engine_with(P1, 50)
    eng.load_batch(seqs, quals)
    names = eng.describe()["node"]
    got = eng.mea_alignments(x, 2.0, 2, profile=True, world="motif")
    none = eng.mea_alignments(x, 2.0, 2, world="none")
    for k, (g, ref) in enumerate(zip(got, refs)):
        L = len(seqs[k])
        assert len(none[k]["start"]) == 0, k      # (every base on node 0: no site)
        if not np.isfinite(ref["Zari"]):
            assert len(g["start"]) == 0 and np.array_equal(g["profile"], nc.no_parse_profile(L, eng.n_node)), k
            continue
        prof = np.clip(ref["motif"]["nodes"], 0.0, 1.0)
        mc.check_result(g, prof, names, 2.0, 2, what=(k, L))
        mc.check_result(g, prof, names, 2.0, 2, own_prof=g["profile"], what=(k, L, "own"))
        assert len(g["start"]) >= 1, k      # (every parse of this world carries the motif)


# ---- 11. the command line

def test_command_line_writes_two_products_of_the_motif_world(tmp_path):
    fq, model = gpath("positive_head6.fq"), gpath("trna_a.model")
    outs = {w: [str(tmp_path / ("%s.%s" % (n, w))) for n in ("a.raw", "context.txt", "access.txt", "contrast.txt")] for w in ("mixed", "motif")}
    for w, (a1, cx, ac_, cf) in outs.items():
        cli.main(["scan", "-f", fq, "-q", model, "--out1", a1, "--out-context", cx, "--out-access", ac_, "--access-width", "4",
                  "--out-contrast", cf, "--chunk", "4"] + (["--world", w] if w != "mixed" else []))
    recs = io.read_fastq(fq)
    m = io.read_model(model)
    eng = io.engine_from_model(m)
    eng.load_batch([s for _, s, _ in recs], [q for _, _, q in recs])
    ctx = eng.context_profiles(m["x"], world="motif")
    acc = eng.accessibility(m["x"], 4, world="motif")
    for k, path in ((1, outs["motif"][1]), (2, outs["motif"][2])):
        lines = open(path).read().split("\n")
        assert lines[0] == "# world: motif" and not open(outs["mixed"][k]).read().startswith("#")
        assert len(lines) == len(open(outs["mixed"][k]).read().split("\n")) + 1
    # the records behind the line are the engine's in that world, in today's format (the printed 6 digits)
    body = open(outs["motif"][1]).read().split("\n", 1)[1]
    want = "".join(io.context_record(rid, ctx[k]) for k, (rid, _, _) in enumerate(recs))
    assert [l.split()[:1] for l in body.split("\n")] == [l.split()[:1] for l in want.split("\n")]
    nums = lambda text: np.array([float(t) for t in text.split() if t.replace(".", "").replace("e-", "").replace("-", "").isdigit()])
    np.testing.assert_allclose(nums(body), nums(want), rtol=2e-6, atol=1e-12)
    body = open(outs["motif"][2]).read().split("\n", 1)[1]
    want = "".join(io.access_record(rid, acc[k]) for k, (rid, _, _) in enumerate(recs))
    np.testing.assert_allclose(nums(body), nums(want), rtol=2e-6, atol=1e-12)
    assert body != open(outs["mixed"][2]).read()
    # the scan records and the contrast file do not depend on the world (up to the rounding of two runs in the printed digits)
    for k in (0, 3):
        a, b = open(outs["mixed"][k]).read(), open(outs["motif"][k]).read()
        assert not b.startswith("#") and len(a.split("\n")) == len(b.split("\n"))
        np.testing.assert_allclose(nums(a), nums(b), rtol=2e-6, atol=1e-9)


# ---- 12. refusals

def test_refusals():
    EINVAL = -1
    lib = api.load_library()
    seqs, quals = batch((20, 31), seed=1, neg_every=0)
    eng = engine_with(P1, 50)
    eng.load_batch(seqs, quals)
    x = perturbed(eng)
    eng.set_option("world", 2)
    for bad in (3.0, -1.0, 1.5, float("nan")):
        assert lib.elemdp_set_option(eng._h, b"world", bad) == EINVAL
    assert eng.world == "none"
    # the refused values changed nothing: a raw call still runs in the world without the motif (a method without world= is "mixed")
    dp = C.POINTER(C.c_double)
    m = C.c_int64()
    unp = np.zeros(int(eng._off[-1]))
    assert lib.elemdp_pair_posteriors(eng._h, x.ctypes.data_as(dp), eng.n_param, 0.0, C.byref(m), unp.ctypes.data_as(dp)) == 0
    got = eng._pair_lists(m.value, unp)
    con = eng.conditional_pairs(x, 0.0)
    for k in range(len(seqs)):
        np.testing.assert_allclose(got[k][2], con[k]["p_none"], rtol=0, atol=1e-12)
        assert np.abs(con[k]["p_none"] - con[k]["p_motif"]).max() > 0.01
    mixed = eng.pair_posteriors(x, 0.0)
    assert np.abs(mixed[1][2] - got[1][2]).max() > 1e-3 and eng.world == "none"
    for name in WORLD_METHODS:
        args = (x, 5) if name == "sample_structures" else (x,)
        with pytest.raises(ValueError):
            getattr(eng, name)(*args, world="both")
    assert eng.world == "none"
    assert lib.elemdp_pair_posteriors(eng._h, x.ctypes.data_as(dp), eng.n_param, -1.0, C.byref(m), None) == EINVAL      # (as in world 0)
