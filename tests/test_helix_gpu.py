"""Helix posteriors on the GPU: Engine.helix_posteriors against the enumeration with the oracle on the
enumerated cases of tests/helix_check.py, against the definition over the oracle's tables at the shapes where the kernels have
code of their own, against the CPU driver of the product rule at lengths that cross the tiles of the list stage and on an automaton
of more than 64 interval states, against the engine's own pair list, across groupings, streamed batches and thresholds, with the
stems of caller-given structures, and through `scan --out-helices --out-mea-helices`."""
import ctypes as C

import numpy as np
import pytest

from rnaelem_amd import api, cli, io
from tests import ctx_check as cc
from tests import helix_check as hc
from tests import large_automata as la
from tests.test_ctx_gpu import pool_map
from tests.test_pair_shapes_gpu import P1, PAR, batch
from tests.util import gpath

pytestmark = pytest.mark.gpu
P5 = "(.....)"
KMAX = 10                   # max_len of the shape cases: no reference of theirs reaches it
PIPELINE3 = (("pipeline", 3),)
_REFS = {}


def cached(key, compute):
    """the references of a case, computed once for the scaled-linear and the log-space form (the oracle is the slow part)"""
    if key not in _REFS:
        _REFS[key] = compute()
    return _REFS[key]


def oracle_with(pattern, x, W=50, C=30):
    def make():
        o = hc.helix_oracle(pattern, W, C)
        o.set_params(x)
        return o
    return make


def table_refs(make, seqs, quals, x, tau=0.1, kmax=KMAX):
    """the table H of every sequence, computed in a pool, longest first"""
    order = sorted(range(len(seqs)), key=lambda k: -len(seqs[k]))
    got = pool_map(make, lambda o, k: hc.table_helices(o, seqs[k], quals[k], x, tau=tau, kmax=kmax), order)
    out = [None] * len(seqs)
    for k, v in zip(order, got):
        out[k] = v
    return out


def engine_with(pattern, W, opts=(), min_bpp=1e-4, flags=0):
    eng = api.Engine(pattern, PAR, W, 30, min_bpp, 0.1, flags, 0)
    for k, v in opts:
        eng.set_option(k, v)
    return eng


def check_helices(eng, x, seqs, refs, kmax=KMAX, what="", log=False):
    """the full list (min_prob 0, min_len 1) against the dense reference, entry by entry, and nothing listed where the reference
    has nothing; the order and the lengths of the list; the properties; no parse: no entries; min_prob = inf keeps none"""
    lists = eng.helix_posteriors(x, 0.0, 1, kmax)
    assert len(lists) == len(seqs)
    dense = []
    for k, (lst, ref) in enumerate(zip(lists, refs)):
        L = len(seqs[k])
        hc.assert_list_order(L, lst, 1, kmax, what=(what, k))
        g = hc.dense_from_list(L, kmax, lst)
        dense.append(g)
        if ref is None:
            assert len(lst[3]) == 0, (what, k)
            continue
        assert not ref[:, :, kmax:].any(), (what, k)          # (the reference fits the bound of the call)
        hc.assert_helix(g, ref[:, :, :kmax], what=(what, k, L))
        hc.assert_properties(g, 1e-10 if log else 1e-12, what=(what, k))
    m = C.c_int64(-1)
    dp = C.POINTER(C.c_double)
    lib = api.load_library()
    assert lib.elemdp_helix_posteriors(eng._h, np.ascontiguousarray(x).ctypes.data_as(dp), eng.n_param, kmax, 1, np.inf, C.byref(m),
                                       None, None, None) == 0
    assert m.value == 0 and lib.elemdp_helix_list(eng._h, None, None, None, None, None, 0) == 0
    return lists, dense


# ---- the enumerated cases

@pytest.mark.parametrize("opts", [(), (("fast", 0),), PIPELINE3], ids=["default", "fast0", "pipeline3"])
def test_enumerated_cases(opts):
    for case in hc.CASES:
        pattern, L, flags, min_bpp = case
        x, s, q, o, enum = hc.tiny_reference(case)
        eng = engine_with(pattern, 50, opts, min_bpp, flags)
        eng.load_batch([s], [q])
        assert enum is not None
        check_helices(eng, x, [s], [enum], kmax=hc.KMAX, what=(opts, case), log=opts == PIPELINE3)
        assert eng.last_timing()[2] == 0      # (no sequence handed on by the range check; pipeline 3 runs none)


# ---- shapes against the definition over the oracle's tables

def shape_case(pattern, W, lens):
    def compute():
        seqs, quals = batch(lens, seed=1000 * W + len(pattern) + len(lens))
        x = hc.helix_params(engine_with(pattern, W))
        return seqs, quals, x, table_refs(oracle_with(pattern, x, W), seqs, quals, x)
    return cached(("shape", pattern, W, lens), compute)


W20_LENS, W70_LENS = tuple(range(1, 61)), (107,)
SHAPES = [(P1, 20, W20_LENS), (P5, 20, W20_LENS), (P1, 70, W70_LENS)]


@pytest.mark.parametrize("log", [False, True], ids=["lin", "pipeline3"])
@pytest.mark.parametrize("pattern,W,lens", SHAPES, ids=["P1-W20", "P5-W20", "P1-W70"])
def test_shapes_against_the_table_definition(pattern, W, lens, log):
    """(L = 1 .. 60: sequences shorter than a pair, than the motif and than W, unit counts from 0 up, rows shorter and longer than
    W; L = 107 at W = 70: chains of up to ten steps, several workgroups of k_helix_chains per sequence)"""
    seqs, quals, x, refs = shape_case(pattern, W, lens)
    eng = engine_with(pattern, W, PIPELINE3 if log else ())
    eng.load_batch(seqs, quals)
    _, dense = check_helices(eng, x, seqs, refs, what=(pattern, W, log), log=log)
    if log:
        assert eng.last_timing()[2] == 0
    assert sum(r is not None for r in refs) >= len(lens) - 1
    assert max(g[:, :, 2].max() for g in dense) > 0.05


def long_case():
    """L = 257 and 300 at W = 20, the references from the CPU driver of the product rule"""
    def compute():
        seqs, quals = batch((257, 300), seed=77, n_every=0)
        x = hc.helix_params(engine_with(P1, 20))
        drv = hc.HelixDriver(P1, PAR, 20, 30, 1e-4, 0.1, 0)
        return seqs, quals, x, [drv.helices(x, s, q, 0, kmax=KMAX)[0] for s, q in zip(seqs, quals)]
    return cached("long", compute)


@pytest.mark.parametrize("log", [False, True], ids=["lin", "pipeline3"])
def test_long_sequences_against_the_cpu_driver(log):
    """L = 257 and 300 at W = 20 cross the tiles of 256 rows of k_helix_units and of 256 units of k_helix_seq"""
    seqs, quals, x, refs = long_case()
    eng = engine_with(P1, 20, PIPELINE3 if log else ())
    eng.load_batch(seqs, quals)
    lists, _ = check_helices(eng, x, seqs, refs, what=("long", log), log=log)
    assert min(len(np.unique(l[0] * 1000 + l[1])) for l in lists) > 256       # (more units than one tile)


def test_an_automaton_of_more_than_64_states():
    """S = 65: the states are strided over the lanes of a wave, two on lane 0.  Planted hairpins of L 57 and 60, against the CPU
    driver; both forms"""
    S = 65
    def compute():
        seqs, quals = la.mixed((57, 60), seed=4100 + S)
        x = hc.helix_params(api.Engine(la.PATTERN[S], PAR, 50, 30, 1e-4, 0.1, 0, 0))
        drv = hc.HelixDriver(la.PATTERN[S], PAR, 50, 30, 1e-4, 0.1, 0)
        return seqs, quals, x, [drv.helices(x, s, q, 0, kmax=KMAX)[0] for s, q in zip(seqs, quals)]
    seqs, quals, x, refs = cached("S65", compute)
    for log in (False, True):
        eng = engine_with(la.PATTERN[S], 50, PIPELINE3 if log else ())
        assert eng.describe()["S"] == S
        eng.load_batch(seqs, quals)
        _, dense = check_helices(eng, x, seqs, refs, what=("S65", log), log=log)
        assert max(g[:, :, 4].max() for g in dense) > 0.05          # (the planted stems: helices of five pairs and more)


# ---- a stem longer than max_len, and the stems of caller-given structures

def hairpin_case():
    def compute():
        s = np.array([3] * 12 + [1] * 4 + [2] * 12, dtype=np.uint8)
        _, (q,) = batch((28,), seed=28, n_every=0, neg_every=0)
        x = hc.helix_params(engine_with(P1, 50))
        return s, q, x, hc.table_helices(oracle_with(P1, x)(), s, q, x, kmax=14)
    return cached("hairpin", compute)


@pytest.mark.parametrize("log", [False, True], ids=["lin", "pipeline3"])
def test_a_stem_longer_than_max_len(log):
    """12 G, AAAA, 12 C with max_len 8, the hairpin twice in the batch: the list stops at len 8; the stem output for the MEA
    structure reports the full length with the value of the table definition; for a stem of length <= max_len the stem output
    equals the list entry of the same call, bit for bit"""
    s, q, x, ref = hairpin_case()
    eng = engine_with(P1, 50, PIPELINE3 if log else ())
    eng.load_batch([s, s], [q, q])
    mea = eng.mea_structures(x, 1.0)[0][0]
    stems = api.structure_helices(mea)
    i0, j0, n0 = max(stems, key=lambda t: t[2])
    assert n0 > 8, mea
    short = ["."] * 28                       # the three innermost pairs of the long stem alone: a stem of three
    for t in range(n0 - 3, n0):
        short[i0 + t], short[j0 - 1 - t] = "(", ")"
    lists, got = eng.helix_posteriors(x, 0.0, 1, 8, structures=[mea, "".join(short)])
    assert lists[0][2].max() == 8 and ((lists[0][0] == i0) & (lists[0][1] == j0) & (lists[0][2] == 8)).sum() == 1
    hc.assert_helix(hc.dense_from_list(28, 8, lists[0]), ref[:, :, :8], what="list")
    si, sj, sn, sp = got[0]
    assert [(int(a), int(b), int(c)) for a, b, c in zip(si, sj, sn)] == stems
    hc.assert_helix(sp, [ref[a, b, c - 1] for a, b, c in stems], what="MEA stems")
    assert 0.0 < sp[stems.index((i0, j0, n0))] < lists[0][3][(lists[0][0] == i0) & (lists[0][1] == j0) & (lists[0][2] == 8)][0]
    si, sj, sn, sp = got[1]
    assert (list(si), list(sj), list(sn)) == ([i0 + n0 - 3], [j0 - n0 + 3], [3])
    ii, jj, kk, pp = lists[1]
    assert sp[0] == pp[(ii == si[0]) & (jj == sj[0]) & (kk == 3)][0] > 0.0                  # bit for bit


def test_a_structure_whose_pair_is_not_kept_gives_zero():
    seqs, quals = batch((60, 33), seed=9, n_every=0, neg_every=0)
    eng = engine_with(P1, 20)
    eng.load_batch(seqs, quals)
    x = hc.helix_params(eng)
    kept = [np.zeros((len(s), len(s) + 1), dtype=bool) for s in seqs]
    for k, (ii, jj, _, _) in enumerate(eng.pair_posteriors(x, 0.0)):
        kept[k][ii, jj] = True
    far = "(" + "." * 58 + ")"                                        # a span above max_span
    a, b = next((i, j) for i in range(33) for j in range(i + 6, 33) if not kept[1][i, j + 1])
    near = "".join("(" if p == a else ")" if p == b else "." for p in range(33))      # a cell the filter did not keep
    for opts in ((), PIPELINE3):
        eng = engine_with(P1, 20, opts)
        eng.load_batch(seqs, quals)
        _, stems = eng.helix_posteriors(x, np.inf, 1, 4, structures=[far, near])
        assert [tuple(int(v[0]) for v in st[:3]) for st in stems] == [(0, 60, 1), (a, b + 1, 1)]
        assert stems[0][3][0] == 0.0 and stems[1][3][0] == 0.0 and not np.signbit(stems[0][3][0])


# ---- models, both forms in one call, no parse, several sequences per workgroup

MODELS = ["syn_sm.model", "syn_a2007.model", "2.model"]


def model_case(model):
    def compute():
        m = io.read_model(gpath(model))
        seqs, quals = batch((3, 13, 40, 97), seed=len(model))
        refs = table_refs(lambda: hc.helix_oracle_from_model(gpath(model))[0], seqs, quals, m["x"], tau=m["tau"], kmax=16)
        return m, seqs, quals, refs
    return cached(("model", model), compute)


@pytest.mark.parametrize("log", [False, True], ids=["lin", "pipeline3"])
@pytest.mark.parametrize("model", MODELS)
def test_models_against_the_table_definition(model, log):
    """softmax theta, the ~A2007~ energy parameters, and a model without secondary structure (2.model: no entries, stem
    probabilities 0, the band tables unread)"""
    m, seqs, quals, refs = model_case(model)
    eng = io.engine_from_model(m)
    for k, v in (PIPELINE3 if log else ()):
        eng.set_option(k, v)
    eng.load_batch(seqs, quals)
    if m["no_rss"]:
        lists, stems = eng.helix_posteriors(m["x"], 0.0, 1, 16, structures=["...", "(" + "." * 11 + ")", "." * 40, "((" + "." * 93 + "))"])
        assert all(len(l[3]) == 0 for l in lists) and all(r is None or not r.any() for r in refs)
        assert [list(st[3]) for st in stems] == [[], [0.0], [], [0.0]] and list(stems[3][2]) == [2]
    else:
        check_helices(eng, m["x"], seqs, refs, kmax=16, what=(model, log), log=log)
    if log:
        assert eng.last_timing()[2] == 0


def test_sequences_out_of_the_double_range_take_the_log_space_form():
    """lambda = 40: the long sequences leave the double range of the scaled-linear tables and go through the fused scan kernel,
    the short ones stay on the scaled-linear path: both forms in one call"""
    recs = io.read_fastq(gpath("syn_L150_n8.fq"))
    short_s, short_q = batch((4, 9, 16, 24), seed=40, neg_every=0)
    seqs = short_s[:2] + [s for _, s, _ in recs][:3] + short_s[2:]
    quals = short_q[:2] + [q for _, _, q in recs][:3] + short_q[2:]
    eng = engine_with(P1, 50, (("group", 2),))
    eng.load_batch(seqs, quals)
    x = eng.initial_params(40.0)
    refs = cached("lambda40", lambda: table_refs(oracle_with(P1, x), seqs, quals, x, kmax=16))
    check_helices(eng, x, seqs, refs, kmax=16, what="lambda 40", log=True)
    structs = eng.mea_structures(x, 1.0)[0]
    lists, stems = eng.helix_posteriors(x, 0.0, 1, 16, structures=structs)
    assert 2 <= eng.last_timing()[2] < len(seqs)
    n = 0
    for k, ((si, sj, sn, sp), ref) in enumerate(zip(stems, refs)):
        hc.assert_helix(sp, [ref[a, b, c - 1] for a, b, c in zip(si, sj, sn)], what=("stems", k))
        n += len(sp)
    assert n > 5


def test_a_sequence_without_any_parse_has_no_helices():
    o = hc.helix_oracle(P1)
    eng = engine_with(P1, 50)
    x, seqs, quals = cc.no_parse_inputs(hc.helix_params(eng), o.hmm())
    eng.load_batch(seqs, quals)
    refs = table_refs(oracle_with(P1, x), seqs, quals, x)
    assert refs[0] is None and refs[1] is not None
    lists, _ = check_helices(eng, x, seqs, refs, what="no parse")
    assert len(lists[0][3]) == 0 and len(lists[1][3]) > 0
    L0 = len(seqs[0])
    db = "(" + "." * (L0 - 2) + ")" if L0 >= 2 else "." * L0
    _, stems = eng.helix_posteriors(x, np.inf, 1, 4, structures=[db, "." * len(seqs[1])])
    assert all(v == 0.0 for v in stems[0][3]) and len(stems[1][3]) == 0


def nine():
    lens = [int(v) for v in np.linspace(20, 160, 9)][::-1]
    lens[2], lens[6] = lens[6], lens[2]
    return batch(lens, seed=5)


def test_a_workgroup_of_the_log_space_form_takes_several_sequences():
    """pipeline 3 with option slots 3: three workgroups take the nine unsorted sequences of L 20 .. 160 off the atomic counter.
    Against the table references, not against another grouping."""
    seqs, quals = nine()
    eng = engine_with(P1, 50, PIPELINE3 + (("slots", 3),))
    eng.load_batch(seqs, quals)
    x = hc.helix_params(eng)
    refs = cached("nine", lambda: table_refs(oracle_with(P1, x), seqs, quals, x, kmax=16))
    check_helices(eng, x, seqs, refs, kmax=16, what="slots 3", log=True)
    assert (eng.slot_status()["slots"], eng.n_seq) == (3, 9)
    assert eng.last_timing()[2] == 0


# ---- identities on one handle

@pytest.mark.parametrize("opts", [(), PIPELINE3], ids=["default", "pipeline3"])
def test_length_one_is_the_pair_list_of_the_same_handle(opts):
    seqs, quals = batch((30, 77, 131), seed=12)
    eng = engine_with(P1, 50, opts)
    eng.load_batch(seqs, quals)
    x = hc.helix_params(eng)
    pairs = eng.pair_posteriors(x, 0.0)
    lists = eng.helix_posteriors(x, 0.0, 1, 16)
    tol = 1e-10 if opts else 1e-12        # (the log-space form: DESIGN.md section 15, Rounding)
    for k, ((pi, pj, pp, _), (ii, jj, kk, p)) in enumerate(zip(pairs, lists)):
        one = kk == 1
        keep = pj - pi >= 2               # (the cells that can hold a pair: every kept cell)
        assert keep.all() and np.array_equal(ii[one], pi) and np.array_equal(jj[one], pj), k          # cell for cell
        np.testing.assert_allclose(p[one], pp, rtol=0, atol=tol, err_msg="pairs %d" % k)
        hc.assert_properties(hc.dense_from_list(len(seqs[k]), 16, lists[k]), tol, what=k)           # monotone, the sub-helix bound
    assert max(p[kk >= 3].max() for _, _, kk, p in lists) > 0.05


# ---- groupings, streamed batches, thresholds, and what a call leaves alone

def raw_helix_list(eng, n):
    i32, dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    cols = [np.full(max(n, 1), -1, dtype=np.int32) for _ in range(4)]
    p = np.full(max(n, 1), np.nan)
    assert api.load_library().elemdp_helix_list(eng._h, *[c.ctypes.data_as(i32) for c in cols], p.ctypes.data_as(dp), n) == 0
    return [c[:n] for c in cols] + [p[:n]]


def test_groupings_thresholds_and_what_a_call_leaves_alone():
    seqs, quals = nine()
    base = engine_with(P1, 50)
    base.load_batch(seqs, quals)
    x = hc.helix_params(base)
    lib = api.load_library()
    i32, dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    first = base.pair_posteriors(x, 0.0)
    cond = base.conditional_pairs(x, 1e-3, 1.0)
    _, stem = base.stem_profiles(x, 0.0)
    structs = base.mea_structures(x, 1.0)[0]
    first = base.pair_posteriors(x, 0.0)
    want, want_stems = base.helix_posteriors(x, 0.0, 1, 16, structures=structs)
    n_hel = sum(len(r[3]) for r in want)
    assert n_hel > 0 and sum(len(s[3]) for s in want_stems) > 9
    # the lists of the last pair, conditional and stem call are still those calls'
    again = base._pair_lists(sum(len(r[0]) for r in first), np.concatenate([r[3] for r in first]))
    for a, b in zip(first, again):
        assert all(np.array_equal(u, v) for u, v in zip(a, b))
    n_cond = sum(len(r["i"]) for r in cond)
    cs, ci, cj = (np.full(n_cond, -1, dtype=np.int32) for _ in range(3))
    cm, cn = np.full(n_cond, np.nan), np.full(n_cond, np.nan)
    assert lib.elemdp_pair_conditional_list(base._h, cs.ctypes.data_as(i32), ci.ctypes.data_as(i32), cj.ctypes.data_as(i32),
                                            cm.ctypes.data_as(dp), cn.ctypes.data_as(dp), n_cond) == 0
    assert n_cond > 0 and np.array_equal(ci, np.concatenate([r["i"] for r in cond])) and np.array_equal(cm, np.concatenate([r["p_motif"] for r in cond]))
    n_stem = sum(len(r[3]) for r in stem)
    ss, si, sj, sk = (np.full(n_stem, -1, dtype=np.int32) for _ in range(4))
    sq = np.full(n_stem, np.nan)
    assert lib.elemdp_stem_list(base._h, ss.ctypes.data_as(i32), si.ctypes.data_as(i32), sj.ctypes.data_as(i32), sk.ctypes.data_as(i32),
                                sq.ctypes.data_as(dp), n_stem) == 0
    assert n_stem > 0 and np.array_equal(sk, np.concatenate([r[2] for r in stem])) and np.array_equal(sq, np.concatenate([r[3] for r in stem]))
    # and the helix list survives theirs, bit for bit
    base.pair_posteriors(x, 0.5)
    base.conditional_pairs(x, 0.5, 1.0)
    base.stem_profiles(x, 0.5)
    assert lib.elemdp_helix_list(base._h, None, None, None, None, None, n_hel - 1) == -1     # (its length too)
    hs, hi, hj, hk, hp = raw_helix_list(base, n_hel)
    assert np.array_equal(hs, np.concatenate([np.full(len(r[3]), k, dtype=np.int32) for k, r in enumerate(want)]))
    for col, got in enumerate((hi, hj, hk, hp)):
        assert np.array_equal(got, np.concatenate([r[col] for r in want])), col
    # a finite threshold keeps exactly the entries of the full list at or above it, in order; min_len likewise
    for thr in (1e-3, 0.3):
        got = base.helix_posteriors(x, thr, 1, 16)
        for a, b in zip(got, want):
            assert np.abs(b[3] - thr).min() > 1e-9                # (no entry of this batch lies within rounding of the threshold)
            keep = b[3] >= thr
            assert all(np.array_equal(u, v[keep]) for u, v in zip(a[:3], b[:3]))
            np.testing.assert_allclose(a[3], b[3][keep], rtol=1e-10, atol=1e-14)
        assert 0 < sum(len(a[3]) for a in got) < n_hel
    got = base.helix_posteriors(x, 1e-3, 3, 5)
    for a, b in zip(got, want):
        keep = (b[3] >= 1e-3) & (b[2] >= 3) & (b[2] <= 5)
        assert all(np.array_equal(u, v[keep]) for u, v in zip(a[:3], b[:3]))
        np.testing.assert_allclose(a[3], b[3][keep], rtol=1e-10, atol=1e-14)
    assert sum(len(a[3]) for a in got) > 0
    assert all(len(l[3]) == 0 for l in base.helix_posteriors(x, np.inf))
    for opts in ((("group", 1),), (("group", 3),), (("max_resident", 4),), (("poison", 1),)):
        eng = engine_with(P1, 50, opts)
        eng.load_batch(seqs, quals)
        got, got_stems = eng.helix_posteriors(x, 0.0, 1, 16, structures=structs)
        for k, (g, w) in enumerate(zip(got, want)):
            assert all(np.array_equal(u, v) for u, v in zip(g[:3], w[:3])), (opts, k)
            np.testing.assert_allclose(g[3], w[3], rtol=1e-10, atol=1e-14, err_msg=str((opts, k)))
        for k, (g, w) in enumerate(zip(got_stems, want_stems)):
            assert all(np.array_equal(u, v) for u, v in zip(g[:3], w[:3])), (opts, k)
            np.testing.assert_allclose(g[3], w[3], rtol=1e-10, atol=1e-14, err_msg=str((opts, k)))


# ---- command line

def test_command_line_writes_the_helix_files(tmp_path):
    fq, model = gpath("positive_head6.fq"), gpath("trna_a.model")
    a1, hf, mf = str(tmp_path / "a.raw"), str(tmp_path / "helices.txt"), str(tmp_path / "mea_helices.txt")
    cli.main(["scan", "-f", fq, "-q", model, "--out1", a1, "--out-helices", hf, "--helix-min-prob", "0.05", "--helix-max-len", "6",
              "--out-mea-helices", mf, "--mea-gamma", "2"])
    recs = io.read_fastq(fq)
    m = io.read_model(model)
    eng = io.engine_from_model(m)
    eng.load_batch([s for _, s, _ in recs], [q for _, _, q in recs])
    structs, _, pairs = eng.mea_structures(m["x"], 2.0, 0.0)
    lists, stems = eng.helix_posteriors(m["x"], 0.05, 2, 6, structures=structs)
    got = io.read_helices(hf)
    want = [(rid, int(i), int(j), int(n), p) for (rid, _, _), lst in zip(recs, lists) for i, j, n, p in zip(*lst)]
    assert len(got) == len(want) > 0
    for g, w in zip(got, want):
        assert (g["id"], g["i"], g["j"], g["len"]) == w[:4] and g["p"] == pytest.approx(w[4], rel=1e-5)
    got = io.read_mea_helices(mf)
    want = [(rid, int(i), int(j), int(n), p, api.stem_min_posterior(pairs[k], int(i), int(j), int(n)))
            for k, ((rid, _, _), st) in enumerate(zip(recs, stems)) for i, j, n, p in zip(*st)]
    assert len(got) == len(want) > 0
    for g, w in zip(got, want):
        assert (g["id"], g["i"], g["j"], g["len"]) == w[:4]
        assert g["p"] == pytest.approx(w[4], rel=1e-5) and g["p_min"] == pytest.approx(w[5], rel=1e-5)
        assert g["p"] <= g["p_min"] * (1 + 1e-5)                      # (the pair marginals bound the joint probability from above)
    assert sorted(p.name for p in tmp_path.iterdir()) == ["a.raw", "helices.txt", "mea_helices.txt"]


def test_refusals():
    eng = engine_with(P1, 50)
    lib = api.load_library()
    x = np.zeros(eng.n_param)
    dp, i32 = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    xp = x.ctypes.data_as(dp)
    call = lambda *a: lib.elemdp_helix_posteriors(eng._h, *a)
    assert call(xp, eng.n_param, 16, 2, 0.0, None, None, None, None) == -4                       # ELEMDP_ESTATE: no batch
    seqs, quals = batch((20,), seed=1)
    eng.load_batch(seqs, quals)
    assert lib.elemdp_helix_list(eng._h, None, None, None, None, None, 0) == -4                  # no helix call on this batch yet
    slen, sprob = np.zeros(20, dtype=np.int32), np.zeros(20)
    sl, sp = slen.ctypes.data_as(i32), sprob.ctypes.data_as(dp)
    for bad in ((None, eng.n_param, 16, 2, 0.0, None, None, None, None),                          # ELEMDP_EINVAL: x
                (xp, eng.n_param, 0, 1, 0.0, None, None, None, None), (xp, eng.n_param, 33, 2, 0.0, None, None, None, None),
                (xp, eng.n_param, 16, 0, 0.0, None, None, None, None), (xp, eng.n_param, 4, 5, 0.0, None, None, None, None),
                (xp, eng.n_param, 16, 2, -0.5, None, None, None, None), (xp, eng.n_param, 16, 2, float("nan"), None, None, None, None),
                (xp, eng.n_param, 16, 2, 0.0, None, ("(" * 20).encode(), sl, sp), (xp, eng.n_param, 16, 2, 0.0, None, ("(..)x" * 4).encode(), sl, sp),
                (xp, eng.n_param, 16, 2, 0.0, None, ("(..)." * 4).encode(), None, None)):
        assert call(*bad) == -1, bad
    assert lib.elemdp_helix_list(eng._h, None, None, None, None, None, 0) == -4                  # (a refused call keeps no list)
    m = C.c_int64()
    assert call(xp, eng.n_param, 32, 1, 0.0, C.byref(m), ("(..)." * 4).encode(), sl, None) == 0 and m.value > 0
    assert list(slen[:6]) == [1, 0, 0, 0, 0, 1]
    assert lib.elemdp_helix_list(eng._h, None, None, None, None, None, m.value - 1) == -1        # cap too small
    assert lib.elemdp_helix_list(eng._h, None, None, None, None, None, m.value) == 0
    eng.load_batch(seqs, quals)
    assert lib.elemdp_helix_list(eng._h, None, None, None, None, None, m.value) == -4            # a new batch: no list
