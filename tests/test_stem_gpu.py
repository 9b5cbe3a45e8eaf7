"""Pair posteriors by motif node pair on the GPU: Engine.stem_profiles against the enumeration of structure
x node row with the oracle on the enumerated cases of tests/stem_check.py, against the definition over the oracle's tables at the
shapes where the kernels have code of their own, against the CPU driver of the product rule at lengths that cross the tiles of
the per-sequence stages, against the oracle's scan, against the engine's own pair list and joint counts, across groupings and
streamed batches, and through `scan --out-stems --out-stem-pairs`."""
import ctypes as C

import numpy as np
import pytest

from rnaelem_amd import api, cli, io
from tests import ctx_check as cc
from tests import stem_check as sc
from tests.test_ctx_gpu import pool_map
from tests.test_pair_shapes_gpu import P1, PAR, batch
from tests.util import gpath

pytestmark = pytest.mark.gpu
P5 = "(.....)"


def oracle_with(pattern, x, W=50, C=30):
    def make():
        o = sc.stem_oracle(pattern, W, C)
        o.set_params(x)
        return o
    return make


def table_refs(make, seqs, quals, x, tau=0.1):
    """the table Q of every sequence, computed in a pool, longest first"""
    order = sorted(range(len(seqs)), key=lambda k: -len(seqs[k]))
    got = pool_map(make, lambda o, k: sc.table_stems(o, seqs[k], quals[k], x, tau=tau), order)
    out = [None] * len(seqs)
    for k, v in zip(order, got):
        out[k] = v
    return out


def check_stems(eng, x, seqs, refs, what="", oracle=None, quals=None):
    """every entry of the full list against the reference; entries in [0, 1]; the list in (i, j, slot) order with every slot of a
    cell; no parse: no entries and counts 0; the counts against the sums of the list; min_prob = inf gives the same counts and no
    list; with an oracle, the counts by pair type against its scan (reference C)"""
    slots = eng.stem_slots()
    K = len(slots)
    counts, lists = eng.stem_profiles(x, 0.0)
    assert counts.shape == (len(seqs), K, 5, 5) and len(lists) == len(seqs)
    dense = []
    for k, (lst, ref) in enumerate(zip(lists, refs)):
        L = len(seqs[k])
        ii, jj, kk, q = lst
        g = sc.dense_from_list(L, K, lst)
        dense.append(g)
        if ref is None:
            assert len(q) == 0 and not counts[k].any(), (what, k)
            continue
        assert len(q) % K == 0 and np.array_equal(kk, np.tile(np.arange(K), len(q) // K)), (what, k)
        key = (ii.astype(np.int64) * (L + 1) + jj) * K + kk
        assert np.all(np.diff(key) > 0), (what, k)
        sc.assert_stem(g, sc.by_slot(ref, slots) if ref.ndim == 4 else ref, what=(what, k, L))
        assert g.min() >= 0.0 and g.max() <= 1.0, (what, k)
        np.testing.assert_allclose(counts[k], sc.counts_of(g, seqs[k]), rtol=1e-13, atol=1e-13 * max(L, 1), err_msg=str((what, k, "counts")))
        if oracle is not None:
            sc.assert_counts_equal_en(oracle, seqs[k], quals[k], counts[k], slots, what=(what, k))
    m = C.c_int64(-1)
    again = np.zeros(max(counts.size, 1))
    dp = C.POINTER(C.c_double)
    assert api.load_library().elemdp_stem_profile(eng._h, np.ascontiguousarray(x).ctypes.data_as(dp), eng.n_param, np.inf,
                                                  again.ctypes.data_as(dp), C.byref(m)) == 0
    assert m.value == 0
    np.testing.assert_allclose(again[:counts.size].reshape(counts.shape), counts, rtol=1e-10, atol=1e-14)
    return counts, lists, dense


def check_en(make, seqs, quals, refs, counts, slots, what=""):
    """reference C on every sequence of a batch that has a parse: the oracle's scans run in a pool, longest first"""
    order = sorted((k for k in range(len(seqs)) if refs[k] is not None), key=lambda k: -len(seqs[k]))
    seen = pool_map(make, lambda o, k: sc.assert_counts_equal_en(o, seqs[k], quals[k], counts[k], slots, what=(what, k)), order)
    assert len(seen) == len(order) and all(v > 0 for v in seen), what


# ---- the enumerated cases

@pytest.mark.parametrize("opts", [(), (("fast", 0),), (("pipeline", 3),)], ids=["default", "fast0", "pipeline3"])
def test_enumerated_cases(opts):
    for case in sc.CASES:
        pattern, L, flags, min_bpp = case
        x, s, q, o, enum = sc.tiny_reference(case)
        eng = api.Engine(pattern, PAR, 50, 30, min_bpp, 0.1, flags, 0)
        for k, v in opts:
            eng.set_option(k, v)
        eng.load_batch([s], [q])
        assert enum is not None
        check_stems(eng, x, [s], [enum], what=(opts, case), oracle=o, quals=[q])
        assert eng.last_timing()[2] == 0      # (no sequence handed on by the range check; pipeline 3 runs none)


# ---- shapes against the definition over the oracle's tables

PIPELINE3 = (("pipeline", 3),)
_REFS = {}


def cached(key, compute):
    """the references of a case, computed once for the scaled-linear and the log-space form (the oracle is the slow part)"""
    if key not in _REFS:
        _REFS[key] = compute()
    return _REFS[key]


def engine_with(pattern, W, opts=()):
    eng = api.Engine(pattern, PAR, W, 30, 1e-4, 0.1, 0, 0)
    for k, v in opts:
        eng.set_option(k, v)
    return eng


def shape_case(pattern, W, lens):
    """(seqs, quals, x, table references) of a shape case"""
    def compute():
        seqs, quals = batch(lens, seed=1000 * W + len(pattern) + len(lens))
        x = sc.stem_params(engine_with(pattern, W))
        return seqs, quals, x, table_refs(oracle_with(pattern, x, W), seqs, quals, x)
    return cached(("shape", pattern, W, lens), compute)


def long_case():
    """L = 257 and 300 at W = 20, the references from the CPU driver of the product rule"""
    def compute():
        seqs, quals = batch((257, 300), seed=77, n_every=0)
        eng = engine_with(P1, 20)
        x = sc.stem_params(eng)
        drv = sc.StemDriver(P1, PAR, 20, 30, 1e-4, 0.1, 0)
        assert np.array_equal(drv.slots, eng.stem_slots())
        return seqs, quals, x, [drv.stems(x, s, q, 0)[0] for s, q in zip(seqs, quals)]
    return cached("long", compute)


W20_LENS, W70_LENS = tuple(range(1, 61)), (107,)


@pytest.mark.parametrize("pattern,W,lens", [(P1, 20, W20_LENS), (P5, 20, W20_LENS), (P1, 70, W70_LENS)],
                         ids=["P1-W20", "P5-W20", "P1-W70"])
def test_shapes_against_the_table_definition(pattern, W, lens):
    """(L = 1 .. 60: sequences shorter than a pair, than the motif and than W, cell counts that are no multiple of the workgroup,
    rows shorter and longer than W; L = 107 at W = 70: eight thousand cells, thirty workgroups of k_stem_cells)"""
    seqs, quals, x, refs = shape_case(pattern, W, lens)
    eng = engine_with(pattern, W)
    eng.load_batch(seqs, quals)
    counts, _, dense = check_stems(eng, x, seqs, refs, what=(pattern, W))
    check_en(oracle_with(pattern, x, W), seqs, quals, refs, counts, eng.stem_slots(), what=(pattern, W))
    assert sum(r is not None for r in refs) >= len(lens) - 1
    assert max(g.sum() for g in dense) > 1.0


@pytest.mark.parametrize("W,lens", [(20, W20_LENS), (70, W70_LENS)], ids=["P1-W20", "P1-W70"])
def test_shapes_in_the_log_space_form(W, lens):
    """pipeline 3: k_dp<DP_SCAN> and StemLog fill the cells the list stage compacts, addressed by launch position; the
    references and the checks of the scaled-linear cases"""
    seqs, quals, x, refs = shape_case(P1, W, lens)
    eng = engine_with(P1, W, PIPELINE3)
    eng.load_batch(seqs, quals)
    counts, _, dense = check_stems(eng, x, seqs, refs, what=(W, "pipeline 3"))
    assert eng.last_timing()[2] == 0
    check_en(oracle_with(P1, x, W), seqs, quals, refs, counts, eng.stem_slots(), what=(W, "pipeline 3"))
    assert sum(r is not None for r in refs) >= len(lens) - 1
    assert max(g.sum() for g in dense) > 1.0


def test_long_sequences_against_the_cpu_driver():
    """L = 257 and 300 at W = 20 cross the tiles of 256 rows of the list kernel"""
    seqs, quals, x, refs = long_case()
    eng = engine_with(P1, 20)
    eng.load_batch(seqs, quals)
    o = oracle_with(P1, x, 20)()
    check_stems(eng, x, seqs, refs, what="long", oracle=o, quals=quals)


def test_long_sequences_in_the_log_space_form():
    """the same under pipeline 3"""
    seqs, quals, x, refs = long_case()
    eng = engine_with(P1, 20, PIPELINE3)
    eng.load_batch(seqs, quals)
    o = oracle_with(P1, x, 20)()
    check_stems(eng, x, seqs, refs, what="long, pipeline 3", oracle=o, quals=quals)
    assert eng.last_timing()[2] == 0


# ---- the identities against the handle's own calls

@pytest.mark.parametrize("opts", [(), (("pipeline", 3),)], ids=["default", "pipeline3"])
def test_sums_are_the_pair_posteriors_and_the_joint_counts_of_the_same_handle(opts):
    seqs, quals = batch((30, 77, 131), seed=12)
    eng = api.Engine(P1, PAR, 50, 30, 1e-4, 0.1, 0, 0)
    for k, v in opts:
        eng.set_option(k, v)
    eng.load_batch(seqs, quals)
    x = sc.stem_params(eng)
    pairs = eng.pair_posteriors(x, 0.0)
    jcounts = eng.joint_profiles(x)
    counts, lists = eng.stem_profiles(x, 0.0)
    slots = eng.stem_slots()
    K = len(slots)
    tol = 1e-10 if opts else 1e-12        # (the log-space form: DESIGN.md section 15, Rounding)
    for k, ((pi, pj, pp, _), (ii, jj, kk, q)) in enumerate(zip(pairs, lists)):
        assert np.array_equal(ii[::K], pi) and np.array_equal(jj[::K], pj), k          # (the same cells)
        np.testing.assert_allclose(q.reshape(-1, K).sum(axis=1), pp, rtol=0, atol=tol, err_msg="pairs %d" % k)
        for m in range(eng.n_node):
            left = counts[k][slots[:, 0] == m].sum(axis=(0, 2)) if (slots[:, 0] == m).any() else np.zeros(5)
            right = counts[k][slots[:, 1] == m].sum(axis=(0, 1)) if (slots[:, 1] == m).any() else np.zeros(5)
            np.testing.assert_allclose(left, jcounts[k, m, 1], rtol=0, atol=tol, err_msg="L %d %d" % (k, m))
            np.testing.assert_allclose(right, jcounts[k, m, 2], rtol=0, atol=tol, err_msg="R %d %d" % (k, m))
    assert max(q.max() for _, _, _, q in lists) > 0.05


MODELS = ["syn_sm.model", "syn_a2007.model", "2.model"]


def model_case(model):
    def compute():
        m = io.read_model(gpath(model))
        seqs, quals = batch((3, 13, 40, 97), seed=len(model))
        refs = table_refs(lambda: sc.stem_oracle_from_model(gpath(model))[0], seqs, quals, m["x"], tau=m["tau"])
        return m, seqs, quals, refs
    return cached(("model", model), compute)


def check_model(model, opts):
    m, seqs, quals, refs = model_case(model)
    eng = io.engine_from_model(m)
    for k, v in opts:
        eng.set_option(k, v)
    eng.load_batch(seqs, quals)
    x = m["x"]
    if m["no_rss"]:
        counts, lists = eng.stem_profiles(x, 0.0)
        assert not counts.any() and all(len(l[3]) == 0 for l in lists)
        assert all(r is None or not r.any() for r in refs)
        return eng
    o = sc.stem_oracle_from_model(gpath(model))[0]
    check_stems(eng, x, seqs, refs, what=(model, opts), oracle=o, quals=quals)
    return eng


@pytest.mark.parametrize("model", MODELS)
def test_models_against_the_table_definition(model):
    """softmax theta, the ~A2007~ energy parameters, and a model without secondary structure (2.model: no stems at all)"""
    check_model(model, ())


@pytest.mark.parametrize("model", MODELS)
def test_models_in_the_log_space_form(model):
    """pipeline 3 (2.model: the no_rss branches of k_dp, stm.has = 0)"""
    eng = check_model(model, PIPELINE3)
    assert eng.last_timing()[2] == 0


def test_sequences_out_of_the_double_range_take_the_log_space_form():
    """lambda = 40: the long sequences leave the double range of the scaled-linear tables and go through the fused scan kernel,
    the short ones stay on the scaled-linear path: both forms in one call"""
    recs = io.read_fastq(gpath("syn_L150_n8.fq"))
    short_s, short_q = batch((4, 9, 16, 24), seed=40, neg_every=0)
    seqs = short_s[:2] + [s for _, s, _ in recs][:3] + short_s[2:]
    quals = short_q[:2] + [q for _, _, q in recs][:3] + short_q[2:]
    eng = api.Engine(P1, PAR, 50, 30, 1e-4, 0.1, 0, 0)
    eng.set_option("group", 2)
    eng.load_batch(seqs, quals)
    x = eng.initial_params(40.0)
    refs = table_refs(oracle_with(P1, x), seqs, quals, x)
    counts, lists, _ = check_stems(eng, x, seqs, refs, what="lambda 40")
    check_en(oracle_with(P1, x), seqs, quals, refs, counts, eng.stem_slots(), what="lambda 40")
    assert 2 <= eng.last_timing()[2] < len(seqs)
    pairs = eng.pair_posteriors(x, 0.0)
    K = len(eng.stem_slots())
    for k, ((pi, pj, pp, _), (ii, jj, kk, q)) in enumerate(zip(pairs, lists)):
        assert np.array_equal(ii[::K], pi) and np.array_equal(jj[::K], pj), k
        np.testing.assert_allclose(q.reshape(-1, K).sum(axis=1), pp, rtol=0, atol=1e-10, err_msg="pairs %d" % k)


def test_a_sequence_without_any_parse_has_no_stems():
    o = sc.stem_oracle(P1)
    eng = api.Engine(P1, PAR, 50, 30, 1e-4, 0.1, 0, 0)
    x, seqs, quals = cc.no_parse_inputs(sc.stem_params(eng), o.hmm())
    eng.load_batch(seqs, quals)
    refs = table_refs(oracle_with(P1, x), seqs, quals, x)
    assert refs[0] is None and refs[1] is not None
    counts, lists, _ = check_stems(eng, x, seqs, refs, what="no parse")
    assert not counts[0].any() and len(lists[0][3]) == 0 and len(lists[1][3]) > 0


def test_a_workgroup_of_the_log_space_form_takes_several_sequences():
    """pipeline 3 with option slots 3: log_scan_args asks for min(slots, n_seq) table slots and launches as many workgroups, so
    n_blocks = 3 workgroups take the n_seq = 9 unsorted sequences of L 20 .. 160 of the grouping test off the atomic counter.
    Against the table references and the oracle's scan, not against another grouping."""
    lens = [int(v) for v in np.linspace(20, 160, 9)][::-1]
    lens[2], lens[6] = lens[6], lens[2]
    seqs, quals = batch(lens, seed=5)
    eng = engine_with(P1, 50, PIPELINE3 + (("slots", 3),))
    eng.load_batch(seqs, quals)
    x = sc.stem_params(eng)
    refs = table_refs(oracle_with(P1, x), seqs, quals, x)
    counts, _, _ = check_stems(eng, x, seqs, refs, what="slots 3")
    assert (eng.slot_status()["slots"], eng.n_seq) == (3, 9)
    assert eng.last_timing()[2] == 0
    check_en(oracle_with(P1, x), seqs, quals, refs, counts, eng.stem_slots(), what="slots 3")
    assert sum(r is not None for r in refs) >= 8


# ---- groupings, streamed batches, thresholds, and what a call leaves alone

def test_groupings_thresholds_and_what_a_call_leaves_alone():
    lens = [int(v) for v in np.linspace(20, 160, 9)][::-1]
    lens[2], lens[6] = lens[6], lens[2]
    seqs, quals = batch(lens, seed=5)
    base = api.Engine(P1, PAR, 50, 30, 1e-4, 0.1, 0, 0)
    base.load_batch(seqs, quals)
    x = sc.stem_params(base)
    first = base.pair_posteriors(x, 0.0)
    cond = base.conditional_pairs(x, 1e-3, 1.0)
    node, jnt = base.node_profiles(x), base.joint_profiles(x)
    want_c, want = base.stem_profiles(x, 0.0)
    again = base._pair_lists(sum(len(r[0]) for r in first), np.concatenate([r[3] for r in first]))
    for a, b in zip(first, again):       # (the list of the last pair call is still the first call's)
        assert all(np.array_equal(u, v) for u, v in zip(a, b))
    # the list of the last conditional call is still that call's, entry by entry, with no conditional call in between
    n_cond = sum(len(r["i"]) for r in cond)
    assert n_cond > 0
    cs, ci, cj = (np.full(n_cond, -1, dtype=np.int32) for _ in range(3))
    cm, cn = np.full(n_cond, np.nan), np.full(n_cond, np.nan)
    i32, dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    assert api.load_library().elemdp_pair_conditional_list(base._h, cs.ctypes.data_as(i32), ci.ctypes.data_as(i32), cj.ctypes.data_as(i32),
                                                           cm.ctypes.data_as(dp), cn.ctypes.data_as(dp), n_cond) == 0
    assert api.load_library().elemdp_pair_conditional_list(base._h, None, None, None, None, None, n_cond - 1) == -1     # (its length too)
    assert np.array_equal(cs, np.concatenate([np.full(len(r["i"]), k, dtype=np.int32) for k, r in enumerate(cond)]))
    assert np.array_equal(ci, np.concatenate([r["i"] for r in cond])) and np.array_equal(cj, np.concatenate([r["j"] for r in cond]))
    assert np.array_equal(cm, np.concatenate([r["p_motif"] for r in cond])) and np.array_equal(cn, np.concatenate([r["p_none"] for r in cond]))
    for a, b in zip(node, base.node_profiles(x)):
        np.testing.assert_allclose(b, a, rtol=1e-10, atol=1e-14)
    np.testing.assert_allclose(base.joint_profiles(x), jnt, rtol=1e-10, atol=1e-14)
    for a, b in zip(first, base.pair_posteriors(x, 0.0)):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        np.testing.assert_allclose(b[2], a[2], rtol=1e-10, atol=1e-14)
    cond2 = base.conditional_pairs(x, 1e-3, 1.0)
    assert len(cond2) == len(cond) == len(seqs)
    for k, (a, b) in enumerate(zip(cond, cond2)):   # (a conditional call after the stem call gives what the one before gave)
        assert np.array_equal(a["i"], b["i"]) and np.array_equal(a["j"], b["j"]), k
        assert (a["structure_motif"], a["structure_none"]) == (b["structure_motif"], b["structure_none"]), k
        for f in ("p_motif", "p_none", "unpaired_motif", "unpaired_none", "exist_prob", "shift"):
            np.testing.assert_allclose(b[f], a[f], rtol=1e-10, atol=1e-14, equal_nan=True, err_msg="%s %d" % (f, k))
    # the list of the last stem call is still that call's, bit for bit, behind pair and conditional calls (the third direction:
    # the three lists share no buffer)
    n_stem = sum(len(r[3]) for r in want)
    assert n_stem > 0
    ss, si, sj, sk = (np.full(n_stem, -1, dtype=np.int32) for _ in range(4))
    sq = np.full(n_stem, np.nan)
    assert api.load_library().elemdp_stem_list(base._h, ss.ctypes.data_as(i32), si.ctypes.data_as(i32), sj.ctypes.data_as(i32),
                                               sk.ctypes.data_as(i32), sq.ctypes.data_as(dp), n_stem) == 0
    assert api.load_library().elemdp_stem_list(base._h, None, None, None, None, None, n_stem - 1) == -1     # (its length too)
    assert np.array_equal(ss, np.concatenate([np.full(len(r[3]), k, dtype=np.int32) for k, r in enumerate(want)]))
    for col, got in enumerate((si, sj, sk, sq)):
        assert np.array_equal(got, np.concatenate([r[col] for r in want])), col
    # a second call on the loaded batch agrees to the last bits (the sum passes add with LDS atomics: DESIGN.md section 12)
    c2, l2 = base.stem_profiles(x, 0.0)
    np.testing.assert_allclose(c2, want_c, rtol=1e-10, atol=1e-14)
    for a, b in zip(l2, want):
        assert all(np.array_equal(u, v) for u, v in zip(a[:3], b[:3]))
        np.testing.assert_allclose(a[3], b[3], rtol=1e-10, atol=1e-14)
    # a finite threshold keeps exactly the entries of the full list at or above it, in order
    for thr in (1e-3, 0.3):
        c3, l3 = base.stem_profiles(x, thr)
        np.testing.assert_allclose(c3, want_c, rtol=1e-10, atol=1e-14)
        for a, b in zip(l3, want):
            keep = b[3] >= thr                                  # (no entry of this batch lies within rounding of a threshold)
            assert all(np.array_equal(u, v[keep]) for u, v in zip(a[:3], b[:3]))
            np.testing.assert_allclose(a[3], b[3][keep], rtol=1e-10, atol=1e-14)
        assert 0 < sum(len(a[3]) for a in l3) < sum(len(b[3]) for b in want)
    assert isinstance(base.stem_profiles(x), np.ndarray)       # (min_prob = inf: the counts alone)
    for opts in ((("group", 1),), (("group", 3),), (("max_resident", 4),), (("poison", 1),)):
        eng = api.Engine(P1, PAR, 50, 30, 1e-4, 0.1, 0, 0)
        for k, v in opts:
            eng.set_option(k, v)
        eng.load_batch(seqs, quals)
        got_c, got = eng.stem_profiles(x, 0.0)
        np.testing.assert_allclose(got_c, want_c, rtol=1e-10, atol=1e-13, err_msg=str(opts))
        for k, (g, w) in enumerate(zip(got, want)):
            assert all(np.array_equal(u, v) for u, v in zip(g[:3], w[:3])), (opts, k)
            np.testing.assert_allclose(g[3], w[3], rtol=1e-10, atol=1e-14, err_msg=str((opts, k)))


# ---- command line

def test_command_line_writes_the_stem_files(tmp_path):
    fq, model = gpath("positive_head6.fq"), gpath("trna_a.model")
    a1, sf, sf2, pf = str(tmp_path / "a.raw"), str(tmp_path / "stems.txt"), str(tmp_path / "stems2.txt"), str(tmp_path / "sp.txt")
    cli.main(["scan", "-f", fq, "-q", model, "--out1", a1, "--out-stems", sf, "--out-stem-pairs", pf, "--stem-min-prob", "0.05"])
    recs = io.read_fastq(fq)
    m = io.read_model(model)
    eng = io.engine_from_model(m)
    eng.load_batch([s for _, s, _ in recs], [q for _, _, q in recs])
    counts, lists = eng.stem_profiles(m["x"], 0.05)
    slots, names = eng.stem_slots(), eng.describe()["node"]
    res, _ = eng.scan(m["x"])
    got = io.read_stems(sf)
    assert (got["n_used"], got["n_total"]) == (len(recs), len(recs)) and np.array_equal(got["slots"], slots)
    np.testing.assert_allclose(got["counts"], api.stem_logo(counts, slots, names)["counts"], rtol=1e-9, atol=1e-12)
    lines = open(pf).read().split("\n")[:-1]
    want = [io.stem_pair_line(rid, i + 1, j, "%d%s" % (slots[t, 0], names[slots[t, 0]]), "%d%s" % (slots[t, 1], names[slots[t, 1]]), q)[:-1]
            for (rid, _, _), lst in zip(recs, lists) for i, j, t, q in zip(*lst)]
    assert len(lines) == len(want) > 0
    for a, b in zip(lines, want):
        fa, fb = a.split("\t"), b.split("\t")
        assert fa[:5] == fb[:5] and float(fa[5]) == pytest.approx(float(fb[5]), rel=1e-5)
    ex = sorted(r["exist_prob"] for r in res)
    cut = 0.5 * (ex[len(ex) // 2 - 1] + ex[len(ex) // 2])
    cli.main(["scan", "-f", fq, "-q", model, "--out1", a1, "--out-stems", sf2, "--logo-min-exist", repr(cut)])
    got2 = io.read_stems(sf2)
    use = np.array([1.0 if r["exist_prob"] >= cut else 0.0 for r in res])
    assert 0 < use.sum() < len(recs) and (got2["n_used"], got2["n_total"]) == (int(use.sum()), len(recs))
    np.testing.assert_allclose(got2["counts"], api.stem_logo(counts, slots, names, use)["counts"], rtol=1e-9, atol=1e-12)
    assert sorted(p.name for p in tmp_path.iterdir()) == ["a.raw", "sp.txt", "stems.txt", "stems2.txt"]


def test_refusals():
    eng = api.Engine(P1, PAR, 50, 30, 1e-4, 0.1, 0, 0)
    lib = api.load_library()
    x = np.zeros(eng.n_param)
    out = np.zeros(25 * len(eng.stem_slots()))
    dp = C.POINTER(C.c_double)
    xp, op = x.ctypes.data_as(dp), out.ctypes.data_as(dp)
    assert lib.elemdp_stem_profile(eng._h, xp, eng.n_param, 0.0, op, None) == -4                   # ELEMDP_ESTATE: no batch
    seqs, quals = batch((20,), seed=1)
    eng.load_batch(seqs, quals)
    assert lib.elemdp_stem_list(eng._h, None, None, None, None, None, 0) == -4                     # no stem call on this batch yet
    assert lib.elemdp_stem_profile(eng._h, xp, eng.n_param, 0.0, None, None) == -1                 # ELEMDP_EINVAL
    assert lib.elemdp_stem_profile(eng._h, None, eng.n_param, 0.0, op, None) == -1
    assert lib.elemdp_stem_profile(eng._h, xp, eng.n_param, -0.5, op, None) == -1
    assert lib.elemdp_stem_profile(eng._h, xp, eng.n_param, float("nan"), op, None) == -1
    m = C.c_int64()
    assert lib.elemdp_stem_profile(eng._h, xp, eng.n_param, 0.0, op, C.byref(m)) == 0 and m.value > 0
    assert lib.elemdp_stem_list(eng._h, None, None, None, None, None, m.value - 1) == -1           # cap too small
    assert lib.elemdp_stem_list(eng._h, None, None, None, None, None, m.value) == 0
    eng.load_batch(seqs, quals)
    assert lib.elemdp_stem_list(eng._h, None, None, None, None, None, m.value) == -4               # a new batch: no list
