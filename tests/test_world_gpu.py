"""Scan posteriors in one world on the GPU: every call that honours option world against the references of
tests/world_check.py -- the enumeration on the tiny cases, the oracle's tables at the lengths around W = 20 and on a batch at W = 50,
with exist_prob near 1 and in mid-range, at W = 70 and at L = 257 and 300, on the softmax, ~A2007~ and no-structure models --, the
mixture identity on the engine's own outputs, the agreement with conditional_pairs, empty worlds under poisoned table slots, both
forms in one call, groupings and a streamed batch (one grouping against another, then slot reuse, two group streams with groups
of more than 64 sequences and several sequences per workgroup of the log-space form against the references), the mixture after a
world call, the sampler, the sites, the command line and the refusals."""
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
from tests.test_loop_gpu import nine
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


W70_LENS = (66, 70, 93, 107)
LONG_LENS = (257, 300)
HEAVY = 3.0

# Two parameter sets.  With the pattern rows raised by HEAVY every sequence that has a parse with the motif has e = exist_prob >= 0.999:
# reference 2 is as well conditioned as it gets, but the world with the motif coincides with the mixture there, so its checks
# cannot tell a launcher that handed the product kernels Z(ari, nasi) in place of Z(ari), or seeded the outside sweep with the
# mixture's terminals, from a right one.  With the rows shifted by MID_SHIFT, chosen per case from the oracle, e lies in mid-range:
# the two worlds and the mixture are three different things, and reference 2 still holds at motif_atol(p, e) = atol (2 - e) / e.
# e of the sequences that have a parse with the motif, in batch order:
#   P1-W20       -1: 0.206, 0.687, 0.714, 0.844
#   P3-W20       -2: 0.0584, 0.467, 0.227, 0.549
#   P1-W50       -2: 0.472, 0.237, 0.427, 0.376, 0.547, 0.0828, 0.0745, 0.448
#   P3-W50       -3: 0.543, 0.266, 0.658, 0.472, 0.619, 0.209, 0.0969, 0.501
#   P1-W70       -2: 0.428, 0.211, 0.299, 0.612
#   P1-W20-long  -2: 0.684, 0.895
# (shift 0 leaves `((.*.))` at e >= 0.94 at W = 20 and e >= 0.999 from L = 66.)
MID_SHIFT = {"P1-W20": -1.0, "P3-W20": -2.0, "P1-W50": -2.0, "P3-W50": -3.0, "P1-W70": -2.0, "P1-W20-long": -2.0}
E_MID = (0.05, 0.95)


def shape_case(pattern, W, lens, shift=HEAVY, products=wc.ALL_PRODUCTS):
    """(seqs, quals, x with the pattern rows shifted -- raised by 3 unless told otherwise --, table references of both worlds)"""
    def compute():
        seqs, quals = batch(lens, seed=31 + W, neg_every=0)
        o = cc.ctx_oracle(pattern, W, 30)
        x = motif_heavy(perturbed(engine_with(pattern, W)), o.hmm(), by=shift)
        return seqs, quals, x, table_refs(pattern, W, x, seqs, quals, products)
    return cached(("shape", pattern, W, lens) if shift == HEAVY else ("shape", pattern, W, lens, shift), compute)


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


MID_SHAPES = [("P1-W20", P1, 20, W20_LENS), ("P3-W20", P3, 20, W20_LENS), ("P1-W50", P1, 50, W50_LENS), ("P3-W50", P3, 50, W50_LENS),
              ("P1-W70", P1, 70, W70_LENS), ("P1-W20-long", P1, 20, LONG_LENS)]


@pytest.mark.parametrize("name,pattern,W,lens", MID_SHAPES, ids=[c[0] for c in MID_SHAPES])
@pytest.mark.parametrize("opts", [(), (("pipeline", 3),)], ids=["lin", "log"])
def test_shapes_with_exist_prob_in_mid_range(name, pattern, W, lens, opts):
    """The shapes above at the parameters of MID_SHIFT, where the world with the motif is not the mixture, and two more: W = 70, a
    band wider than a wave, at L = 66 .. 107, and L = 257 and 300 at W = 20, the second tile of 256 rows of the per-sequence
    kernels.  All eight products everywhere: at W = 20 the table references of accessibility, of the stem profile and of the joint
    profile take under a second per sequence at L = 300 too."""
    products = wc.ALL_PRODUCTS
    seqs, quals, x, refs = shape_case(pattern, W, lens, MID_SHIFT[name], products)
    es = [r["e"] for r in refs if np.isfinite(r["Zari"])]
    print("%s, shift %g: e %s" % (name, MID_SHIFT[name], ["%.3g" % e for e in es]))
    assert all(e >= wc.E_MIN for e in es), es
    assert all(np.isfinite(r["Znasi"]) for r in refs) and len(es) >= len(refs) - 2
    assert 3 * sum(E_MID[0] <= e <= E_MID[1] for e in es) >= len(es) > 0, es
    eng = engine_with(pattern, W, opts)
    eng.load_batch(seqs, quals)
    got = check_worlds(eng, x, seqs, refs, products, what=(name, opts))
    if any(k == "pipeline" for k, _ in opts):
        assert eng.last_timing()[2] == 0
    # (the worlds differ: the mixture in place of the world with the motif cannot pass)
    assert max(np.abs(g["context"] - r["mixed"]["context"]).max() for g, r in zip(got["motif"], refs) if np.isfinite(r["Zari"])) > 0.01


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


def processing_groups(seqs, gsz):
    """group index of every sequence: the engine sweeps the batch longest first (a stable sort) in groups of gsz"""
    order = sorted(range(len(seqs)), key=lambda k: -len(seqs[k]))
    out = [0] * len(seqs)
    for pos, k in enumerate(order):
        out[k] = pos // gsz
    return out


def test_three_slots_reused_by_seven_groups_against_the_references():
    """Option group 3 on 20 unsorted sequences of L 5 .. 200: seven groups reuse three slots, and with them the call's scratch
    and the world's column of zs.  Against the table references, where test_groupings_and_a_streamed_batch_give_the_same_products
    holds one grouping to another (both could be wrong the same way).  Two sequences have an empty motif world, in different
    groups: L = 5, shorter than the pattern, and poly-A of L = 97, which keeps no pair -- k_world_empty flags each behind the
    inside sweep of its own group."""
    lens = [int(v) for v in np.linspace(5, 200, 20)][::-1]
    lens[3], lens[11] = lens[11], lens[3]
    prods = ("pairs", "context", "nodes", "loops", "helices")

    def compute():
        seqs, quals = batch(lens, seed=53, neg_every=0)
        seqs[lens.index(97)] = np.ones(97, dtype=np.uint8)          # (poly-A: no kept pair, so no parse with `((.*.))`)
        x = perturbed(engine_with(P1, 50))
        return seqs, quals, x, table_refs(P1, 50, x, seqs, quals, prods)
    seqs, quals, x, refs = cached("group3", compute)
    empty = [k for k, r in enumerate(refs) if not np.isfinite(r["Zari"])]
    groups = processing_groups(seqs, 3)
    assert sorted(len(seqs[k]) for k in empty) == [5, 97] and groups[empty[0]] != groups[empty[1]] and max(groups) == 6
    assert all(r["e"] >= wc.E_MIN or not np.isfinite(r["Zari"]) for r in refs), [r["e"] for r in refs]
    eng = engine_with(P1, 50, (("group", 3),))
    eng.load_batch(seqs, quals)
    check_worlds(eng, x, seqs, refs, prods, what="group 3")
    eng.pair_posteriors(x, 0.0, world="motif")
    assert eng.last_timing()[2] == len(empty)


@pytest.mark.parametrize("group,gsz", [(128, 54), (256, 80)])
def test_two_group_streams_and_groups_of_more_than_a_wave(group, gsz, monkeypatch, capfd):
    """320 sequences of L 3 .. 60, 100 of them shorter than the pattern (L < 7: an empty motif world), as
    test_two_group_streams_with_three_groups_each of tests/test_pair_shapes_gpu.py: from 128 sequences and 128 slots on, two group
    streams with half the slots each.  Option group 128: six groups of 54 (the last 50), three per stream; option group 256:
    four groups of 80, two per stream, so that k_world_empty runs two workgroups per group, (G + 63) / 64.  The engine sweeps the
    batch longest first, whatever its order, so the short sequences fill the last two groups of the sweep, one on each stream,
    and the batch order cannot put them into every group: both streams append their empty worlds to the one flagged list with
    atomics (under option group 256, lanes of both workgroups of k_world_empty).  From the oracle: 112 empty motif worlds (12
    longer sequences have no parse with the motif either), e >= E_MIN for the other 208.  Pairs and context in the scaled-linear form: the world without the
    motif of every sequence against reference 1, the world with it against reference 2 where e >= E_MIN and against the
    conventions of an empty world, exactly, where it is empty; the flagged counts; a scan afterwards, whose launcher reports the
    groups."""
    prods = ("pairs", "context")

    def compute():
        rng = np.random.default_rng(320)
        lens = np.concatenate([rng.integers(3, 7, size=100), rng.integers(7, 61, size=220)])
        rng.shuffle(lens)
        seqs, quals = batch([int(v) for v in lens], seed=320, neg_every=0)
        x = perturbed(engine_with(P1, 50))
        return seqs, quals, x, table_refs(P1, 50, x, seqs, quals, prods)
    seqs, quals, x, refs = cached("streams", compute)
    n = len(seqs)
    empty = {k for k, r in enumerate(refs) if not np.isfinite(r["Zari"])}
    groups = processing_groups(seqs, gsz)
    assert sum(len(s) < 7 for s in seqs) == 100 and all(k in empty for k in range(n) if len(seqs[k]) < 7)
    assert {groups[k] % 2 for k in empty} == {0, 1}          # (groups are dealt to the two streams in turn)
    assert all(np.isfinite(r["Znasi"]) for r in refs)
    eng = engine_with(P1, 50, (("group", group),))
    eng.load_batch(seqs, quals)
    got, flagged = {}, {}
    for w in WORLDS:
        got[w] = wc.engine_products(eng, x, w, seqs, prods)
        flagged[w] = eng.last_timing()[2]
    assert flagged == dict(motif=len(empty), none=0), (flagged, len(empty))
    M, K = eng.n_node, len(eng.stem_slots())
    compared = 0
    for k, ref in enumerate(refs):
        L = len(seqs[k])
        wc.assert_world(got["none"][k], ref, "none", what=(group, k, L))
        if not np.isfinite(ref["Zari"]):
            check_empty(got["motif"][k], L, min(L, 50), M, K, what=(group, k, L))
        elif ref["e"] >= wc.E_MIN:
            wc.assert_world(got["motif"][k], ref, "motif", what=(group, k, L))
            compared += 1
    print("two group streams, group %d: %d empty motif worlds, %d compared with reference 2" % (group, len(empty), compared))
    assert compared >= 100, compared
    monkeypatch.setenv("ELEMDP_LDS_DEBUG", "1")
    capfd.readouterr()
    recs, _ = eng.scan(x)
    assert len(recs) == n and eng.world == "mixed"
    sizes = [int(line.split()[3]) for line in capfd.readouterr().err.splitlines() if line.startswith("scan group: G ")]
    assert sizes == [gsz] * (n // gsz) + ([n % gsz] if n % gsz else []), sizes


def test_a_workgroup_of_the_log_space_form_takes_several_sequences():
    """pipeline 3 with option slots 3: three workgroups take the nine unsorted sequences of L 20 .. 160 off the atomic counter, in
    both worlds.  Pairs, context and loops against the table references, not against another grouping."""
    prods = ("pairs", "context", "loops")
    seqs, quals = nine()
    x = perturbed(engine_with(P1, 50))
    refs = cached("nine", lambda: table_refs(P1, 50, x, seqs, quals, prods))
    assert all(r["e"] >= wc.E_MIN or not np.isfinite(r["Zari"]) for r in refs), [r["e"] for r in refs]
    assert sum(np.isfinite(r["Zari"]) for r in refs) >= 4
    eng = engine_with(P1, 50, (("pipeline", 3), ("slots", 3)))
    eng.load_batch(seqs, quals)
    check_worlds(eng, x, seqs, refs, prods, what="slots 3")
    assert (eng.slot_status()["slots"], eng.n_seq) == (3, 9)
    assert eng.last_timing()[2] == 0


# ---- 7b. models

MODELS = ["syn_sm.model", "syn_a2007.model", "2.model"]
MODEL_PRODUCTS = ("pairs", "context", "nodes", "loops", "helices")


def model_case(model):
    """(model, seqs, quals, table references of both worlds): reference 1 on cond_check.none_params of the model's x (a softmax
    model's second oracle takes the log-probabilities as plain theta: cond_check.model_oracles)"""
    def compute():
        path = gpath(model)
        m = io.read_model(path)
        # (the seed: reference 2 needs e >= E_MIN.  At seed 3 the sequence of L = 13 has e = 0.605 under syn_sm.model, 0.495 under
        # syn_a2007.model and 0.977 under 2.model, L = 40 and 97 have e >= 0.979; the seed of the other files, len(model), leaves
        # L = 13 at e = 3e-4 under syn_sm.model)
        seqs, quals = batch((3, 13, 40, 97), seed=3, neg_every=0)
        xn = cd.none_params(m["x"], cd.model_oracles(path)[0].hmm(), softmax=m["softmax"])
        order = sorted(range(len(seqs)), key=lambda k: -len(seqs[k]))
        # (without secondary structure the oracle's P plane means nothing -- cond_check.table_worlds has zeros for it too: the
        # test holds the pair call to the empty list instead)
        prods = MODEL_PRODUCTS[1:] if m["no_rss"] else MODEL_PRODUCTS
        got = pool_map(lambda: cd.model_oracles(path),
                       lambda oo, k: wc.table_worlds(oo[0], oo[1], m["x"], xn, seqs[k], quals[k], prods), order)
        refs = [None] * len(seqs)
        for k, v in zip(order, got):
            refs[k] = v
        return m, seqs, quals, refs
    return cached(("model", model), compute)


@pytest.mark.parametrize("opts", [(), (("pipeline", 3),)], ids=["lin", "log"])
@pytest.mark.parametrize("model", MODELS)
def test_models_against_the_tables_of_both_worlds(model, opts):
    """softmax theta, the ~A2007~ energy parameters, and a model without secondary structure (2.model, pattern `..*..`: no pair,
    loop or helix in either world, the lists empty and the counts 0; context and node profiles still against the references).
    L = 3 is shorter than either pattern: an empty motif world."""
    m, seqs, quals, refs = model_case(model)
    assert all(r["e"] >= wc.E_MIN or not np.isfinite(r["Zari"]) for r in refs), [r["e"] for r in refs]
    assert not np.isfinite(refs[0]["Zari"]) and sum(np.isfinite(r["Zari"]) for r in refs) >= 2 and all(np.isfinite(r["Znasi"]) for r in refs)
    eng = io.engine_from_model(m)
    for k, v in opts:
        eng.set_option(k, v)
    eng.load_batch(seqs, quals)
    got = check_worlds(eng, m["x"], seqs, refs, MODEL_PRODUCTS[1:] if m["no_rss"] else MODEL_PRODUCTS, what=(model, opts))
    if m["no_rss"]:
        for w in WORLDS:
            for g, h in zip(got[w], wc.engine_products(eng, m["x"], w, seqs, ("pairs",))):
                assert not h["pairs"].any() and np.all(h["unpaired"] == 1.0) and not g["loops"].any() and not g["helices"].any(), w
                assert not g["loop_counts"].any() and g["two"] == {}, w
        assert max(np.abs(a["nodes"] - b["nodes"]).max() for a, b in zip(got["motif"], got["none"])) > 0.5
    if opts:
        assert eng.last_timing()[2] == 0


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
