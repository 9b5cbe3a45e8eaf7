"""Loop posteriors on the GPU: Engine.loop_posteriors against the enumeration with the oracle on the
enumerated cases of tests/loop_check.py, against the definition over the oracle's tables at the shapes where the kernels have code
of their own, against the CPU driver of the product rule where an outer cell holds more items than a wave has lanes, at lengths
that cross the tiles of the list stage and on an automaton of more than 64 interval states, against the engine's own pair, helix
and context calls, across groupings, streamed batches and thresholds, with the loops of caller-given structures, and through
`scan --out-loops --out-mea-loops`."""
import ctypes as C

import numpy as np
import pytest

from rnaelem_amd import api, cli, io, synth
from tests import ctx_check as cc
from tests import large_automata as la
from tests import loop_check as lc
from tests.test_ctx_gpu import pool_map
from tests.test_pair_shapes_gpu import P1, PAR, batch
from tests.util import gpath

pytestmark = pytest.mark.gpu
P5 = "(.....)"
PIPELINE3 = (("pipeline", 3),)
WAVE = 64                   # lanes of a wave of k_loop_items: an outer cell with more items takes more than one pass
_REFS = {}


def cached(key, compute):
    """the references of a case, computed once for the scaled-linear and the log-space form (the oracle is the slow part)"""
    if key not in _REFS:
        _REFS[key] = compute()
    return _REFS[key]


def oracle_with(pattern, x, W=50, C_=30):
    def make():
        o = lc.loop_oracle(pattern, W, C_)
        o.set_params(x)
        return o
    return make


def table_refs(make, seqs, quals, x, tau=0.1):
    """the table reference (cols, two, P) of every sequence, computed in a pool, longest first"""
    order = sorted(range(len(seqs)), key=lambda k: -len(seqs[k]))
    got = pool_map(make, lambda o, k: lc.table_loops(o, seqs[k], quals[k], x, tau=tau), order)
    out = [None] * len(seqs)
    for k, v in zip(order, got):
        out[k] = v
    return out


def driver_refs(drv, seqs, quals, x):
    out = []
    for s, q in zip(seqs, quals):
        r = drv.loops(x, s, q, 0)
        out.append((r["cols"], r["two"], r["P"]))
    return out


def engine_with(pattern, W, opts=(), min_bpp=1e-4, flags=0):
    eng = api.Engine(pattern, PAR, W, 30, min_bpp, 0.1, flags, 0)
    for k, v in opts:
        eng.set_option(k, v)
    return eng


def check_loops(eng, x, seqs, refs, what="", log=False):
    """the full lists (min_prob 0) against the reference (cols, two[, P]) of every sequence, entry by entry and keyed by
    (i, j, k, l), and nothing listed where the reference has nothing; the order of both lists; the counts; the identities between
    the lists; no parse: no entries; min_prob = inf keeps none"""
    closing, two, counts = eng.loop_posteriors(x, 0.0)
    assert len(closing) == len(two) == len(counts) == len(seqs)
    tol = 1e-10 if log else 1e-12
    for k, ref in enumerate(refs):
        L = len(seqs[k])
        ii, jj, p, cols = closing[k]
        ti, tj, tk, tl, tp = two[k]
        if ref is None:
            assert len(p) == 0 and len(tp) == 0 and not counts[k].any(), (what, k)
            continue
        assert np.all(np.diff(ii.astype(np.int64) * (L + 1) + jj) > 0), (what, k)
        assert cols.size == 0 or (cols.min() >= 0.0 and cols.max() <= 1.0)
        g, gp = lc.dense_from_closing(L, closing[k])
        lc.assert_loop(g, ref[0], what=(what, k, L))
        lc.assert_two(lc.two_dict(two[k]), ref[1], what=(what, k, L))
        if len(ref) > 2:
            lc.assert_loop(gp, ref[2], what=(what, k, "P"))
        # the two-loops follow their outer cells in closing order; the entries of a cell add up to its B + I
        at = {(int(a), int(b)): r for r, (a, b) in enumerate(zip(ii, jj))}
        rows = np.array([at[(int(a), int(b))] for a, b in zip(ti, tj)], dtype=np.int64)
        assert np.all(np.diff(rows) >= 0), (what, k)
        per = np.zeros(len(p))
        np.add.at(per, rows, tp)
        assert np.abs(per - cols[:, lc.B_] - cols[:, lc.I_]).max(initial=0.0) <= tol, (what, k)
        assert np.abs(cols.sum(axis=1) - p).max(initial=0.0) <= tol, (what, k, np.abs(cols.sum(axis=1) - p).max(initial=0.0))
        assert np.abs(counts[k] - cols.sum(axis=0)).max() <= tol * max(1, len(p)), (what, k)
        assert abs(counts[k].sum() - p.sum()) <= tol * max(1, len(p)), (what, k)
    m1, m2 = C.c_int64(-1), C.c_int64(-1)
    dp = C.POINTER(C.c_double)
    lib = api.load_library()
    assert lib.elemdp_loop_posteriors(eng._h, np.ascontiguousarray(x).ctypes.data_as(dp), eng.n_param, np.inf, None, C.byref(m1),
                                      C.byref(m2), None, None, None) == 0
    assert m1.value == 0 and m2.value == 0 and lib.elemdp_loop_closing_list(eng._h, None, None, None, None, None, 0) == 0
    assert lib.elemdp_loop_two_list(eng._h, None, None, None, None, None, None, 0) == 0
    return closing, two, counts


# ---- the enumerated cases

@pytest.mark.parametrize("opts", [(), (("fast", 0),), PIPELINE3], ids=["default", "fast0", "pipeline3"])
def test_enumerated_cases(opts):
    for case in lc.CASES:
        pattern, L, flags, min_bpp = case
        x, s, q, o, enum = lc.tiny_reference(case)
        eng = engine_with(pattern, 50, opts, min_bpp, flags)
        eng.load_batch([s], [q])
        assert enum is not None
        check_loops(eng, x, [s], [enum], what=(opts, case), log=opts == PIPELINE3)
        assert eng.last_timing()[2] == 0      # (no sequence handed on by the range check; pipeline 3 runs none)


# ---- shapes against the definition over the oracle's tables

W20_LENS = tuple(range(1, 61))


def shape_case(pattern, W, lens):
    def compute():
        seqs, quals = batch(lens, seed=2000 * W + len(pattern) + len(lens))
        x = lc.loop_params(engine_with(pattern, W))
        return seqs, quals, x, table_refs(oracle_with(pattern, x, W), seqs, quals, x)
    return cached(("shape", pattern, W, lens), compute)


@pytest.mark.parametrize("log", [False, True], ids=["lin", "pipeline3"])
@pytest.mark.parametrize("pattern", [P1, P5], ids=["P1-W20", "P5-W20"])
def test_shapes_against_the_table_definition(pattern, log):
    """a ragged batch of L = 1 .. 60 at W = 20: sequences shorter than a pair, than the motif and than W, unit counts from 0 up"""
    seqs, quals, x, refs = shape_case(pattern, 20, W20_LENS)
    eng = engine_with(pattern, 20, PIPELINE3 if log else ())
    eng.load_batch(seqs, quals)
    closing, two, _ = check_loops(eng, x, seqs, refs, what=(pattern, log), log=log)
    if log:
        assert eng.last_timing()[2] == 0
    assert sum(r is not None for r in refs) >= len(W20_LENS) - 1
    assert max(c[3][:, lc.H_].max(initial=0.0) for c in closing) > 0.05 and max(t[4].max(initial=0.0) for t in two) > 0.01


# ---- against the CPU driver of the product rule

def wide_case(min_bpp):
    def compute():
        seqs, quals = synth.synth_batch(1, 107, seed=207)
        x = lc.loop_params(engine_with(P1, 70, (), min_bpp))
        drv = lc.LoopDriver(P1, PAR, 70, 30, min_bpp, 0.1, 0)
        return seqs, quals, x, driver_refs(drv, seqs, quals, x)
    return cached(("wide", min_bpp), compute)


@pytest.mark.parametrize("min_bpp", [1e-4, 0.0])
def test_an_outer_cell_with_more_items_than_a_wave_pass(min_bpp):
    """((.*.)), L = 107, W = 70: outer cells of up to 87 items at min_bpp 1e-4 and 234 at 0, two to four passes of the 64 lanes"""
    seqs, quals, x, refs = wide_case(min_bpp)
    per = {}
    for (i, j, _, _) in refs[0][1]:
        per[(i, j)] = per.get((i, j), 0) + 1
    assert max(per.values()) > WAVE, max(per.values())
    assert refs[0][0][:, :, lc.M_].max() > 0.1          # (with energies: the multi-branch column far above the tolerance; seen 0.229)
    eng = engine_with(P1, 70, (), min_bpp)
    eng.load_batch(seqs, quals)
    check_loops(eng, x, seqs, refs, what=("wide", min_bpp))


def long_case():
    def compute():
        seqs, quals = batch((257, 300), seed=78, n_every=0)
        x = lc.loop_params(engine_with(P1, 20))
        drv = lc.LoopDriver(P1, PAR, 20, 30, 1e-4, 0.1, 0)
        return seqs, quals, x, driver_refs(drv, seqs, quals, x)
    return cached("long", compute)


@pytest.mark.parametrize("log", [False, True], ids=["lin", "pipeline3"])
def test_long_sequences_against_the_cpu_driver(log):
    """L = 257 and 300 at W = 20 cross the tiles of 256 rows of the unit compaction and of 256 units of k_loop_seq"""
    seqs, quals, x, refs = long_case()
    eng = engine_with(P1, 20, PIPELINE3 if log else ())
    eng.load_batch(seqs, quals)
    closing, _, _ = check_loops(eng, x, seqs, refs, what=("long", log), log=log)
    assert min(len(c[0]) for c in closing) > 256       # (more units than one tile)


def test_an_automaton_of_more_than_64_states():
    """S = 65: the states of out(E) are strided over the lanes of a wave.  Planted hairpins of L 57 and 60; both forms"""
    S = 65

    def compute():
        seqs, quals = la.mixed((57, 60), seed=4100 + S)
        x = lc.loop_params(api.Engine(la.PATTERN[S], PAR, 50, 30, 1e-4, 0.1, 0, 0))
        drv = lc.LoopDriver(la.PATTERN[S], PAR, 50, 30, 1e-4, 0.1, 0)
        return seqs, quals, x, driver_refs(drv, seqs, quals, x)
    seqs, quals, x, refs = cached("S65", compute)
    for log in (False, True):
        eng = engine_with(la.PATTERN[S], 50, PIPELINE3 if log else ())
        assert eng.describe()["S"] == S
        eng.load_batch(seqs, quals)
        closing, _, _ = check_loops(eng, x, seqs, refs, what=("S65", log), log=log)
        assert max(c[3][:, lc.S_].max() for c in closing) > 0.05          # (the planted stems)


# ---- models, both forms in one call, no parse, several sequences per workgroup

MODELS = ["syn_sm.model", "syn_a2007.model", "2.model"]


def model_case(model):
    def compute():
        m = io.read_model(gpath(model))
        seqs, quals = batch((3, 13, 40, 97), seed=len(model))
        refs = table_refs(lambda: lc.loop_oracle_from_model(gpath(model))[0], seqs, quals, m["x"], tau=m["tau"])
        return m, seqs, quals, refs
    return cached(("model", model), compute)


@pytest.mark.parametrize("log", [False, True], ids=["lin", "pipeline3"])
@pytest.mark.parametrize("model", MODELS)
def test_models_against_the_table_definition(model, log):
    """softmax theta, the ~A2007~ energy parameters, and a model without secondary structure (2.model: nothing listed, counts 0,
    loop probabilities 0, the band tables unread)"""
    m, seqs, quals, refs = model_case(model)
    eng = io.engine_from_model(m)
    for k, v in (PIPELINE3 if log else ()):
        eng.set_option(k, v)
    eng.load_batch(seqs, quals)
    if m["no_rss"]:
        closing, two, counts, loops = eng.loop_posteriors(m["x"], 0.0, structures=["...", "(" + "." * 11 + ")", "." * 40,
                                                                                 "((" + "." * 93 + "))"])
        assert all(len(c[2]) == 0 for c in closing) and all(len(t[4]) == 0 for t in two) and not counts.any()
        assert [list(l[5]) for l in loops] == [[], [0.0], [], [0.0, 0.0]] and list(loops[3][0]) == [2, 1]
    else:
        check_loops(eng, m["x"], seqs, refs, what=(model, log), log=log)
    if log:
        assert eng.last_timing()[2] == 0


def test_sequences_out_of_the_double_range_take_the_log_space_form():
    """lambda = 40: the long sequences leave the double range of the scaled-linear tables and go through the fused scan kernel,
    the short ones stay on the scaled-linear path: both forms in one call; the loops of the MEA structures against the table
    definition"""
    recs = io.read_fastq(gpath("syn_L150_n8.fq"))
    short_s, short_q = batch((4, 9, 16, 24), seed=40, neg_every=0)
    seqs = short_s[:2] + [s for _, s, _ in recs][:3] + short_s[2:]
    quals = short_q[:2] + [q for _, _, q in recs][:3] + short_q[2:]
    eng = engine_with(P1, 50, (("group", 2),))
    eng.load_batch(seqs, quals)
    x = eng.initial_params(40.0)
    refs = cached("lambda40", lambda: table_refs(oracle_with(P1, x), seqs, quals, x))
    check_loops(eng, x, seqs, refs, what="lambda 40", log=True)
    structs = eng.mea_structures(x, 1.0)[0]
    closing, two, _, loops = eng.loop_posteriors(x, 0.0, structures=structs)
    assert 2 <= eng.last_timing()[2] < len(seqs)
    n = 0
    for k, ((lt, li, lj, lk, ll, lp), ref) in enumerate(zip(loops, refs)):
        want = [ref[1].get((i, j, a, b), 0.0) if t in (3, 4) else ref[0][i, j, t - 1] for t, i, j, a, b in zip(lt, li, lj, lk, ll)]
        lc.assert_loop(lp, want, what=("MEA loops", k))
        n += len(lp)
    assert n > 5


def test_a_sequence_without_any_parse_has_no_loops():
    o = lc.loop_oracle(P1)
    eng = engine_with(P1, 50)
    x, seqs, quals = cc.no_parse_inputs(lc.loop_params(eng), o.hmm())
    eng.load_batch(seqs, quals)
    refs = table_refs(oracle_with(P1, x), seqs, quals, x)
    assert refs[0] is None and refs[1] is not None
    closing, _, _ = check_loops(eng, x, seqs, refs, what="no parse")
    assert len(closing[0][2]) == 0 and len(closing[1][2]) > 0
    L0 = len(seqs[0])
    db = "(" + "." * (L0 - 2) + ")" if L0 >= 2 else "." * L0
    loops = eng.loop_posteriors(x, np.inf, structures=[db, "." * len(seqs[1])])[3]
    assert all(v == 0.0 for v in loops[0][5]) and len(loops[1][5]) == 0


def nine():
    lens = [int(v) for v in np.linspace(20, 160, 9)][::-1]
    lens[2], lens[6] = lens[6], lens[2]
    return batch(lens, seed=5)


def nine_refs(x):
    seqs, quals = nine()
    return cached("nine", lambda: table_refs(oracle_with(P1, x), seqs, quals, x))


def test_a_workgroup_of_the_log_space_form_takes_several_sequences():
    """pipeline 3 with option slots 3: three workgroups take the nine unsorted sequences of L 20 .. 160 off the atomic counter.
    Against the table references, not against another grouping."""
    seqs, quals = nine()
    eng = engine_with(P1, 50, PIPELINE3 + (("slots", 3),))
    eng.load_batch(seqs, quals)
    x = lc.loop_params(eng)
    check_loops(eng, x, seqs, nine_refs(x), what="slots 3", log=True)
    assert max(r[0][:, :, lc.M_].max() for r in nine_refs(x)) > 0.02     # (with energies, against the table definition; seen 0.051)
    assert (eng.slot_status()["slots"], eng.n_seq) == (3, 9)
    assert eng.last_timing()[2] == 0


# ---- identities on one handle

@pytest.mark.parametrize("opts", [(), PIPELINE3], ids=["default", "pipeline3"])
def test_identities_with_the_pair_helix_and_context_calls_of_the_same_handle(opts):
    """the closing list row for row against the handle's own pair list at two thresholds: the same cells in the same order, and p
    -- the P plane of the same launch_pair_cells -- at the tolerance of the identities, not bit for bit: two calls sweep the tables
    anew, and the sum passes of two calls do not give the same bits (two pair_posteriors calls on this very handle differ from
    each other by up to 2.2e-16 absolute, 5.8e-16 relative, and so does a loop call from either); S against the len-2
    entries of helix_posteriors; H, the bulge entries and the interior entries range-added against columns H, B, I of
    context_profiles"""
    seqs, quals = batch((30, 77, 131), seed=12)
    eng = engine_with(P1, 50, opts)
    eng.load_batch(seqs, quals)
    x = lc.loop_params(eng)
    tol = 1e-10 if opts else 1e-12        # (the log-space form: DESIGN.md section 15, Rounding)
    for thr in (0.0, 0.01):
        pairs = eng.pair_posteriors(x, thr)
        closing = eng.loop_posteriors(x, thr)[0]
        for k, ((pi, pj, pp, _), (ii, jj, p, _)) in enumerate(zip(pairs, closing)):
            assert np.array_equal(ii, pi) and np.array_equal(jj, pj), (thr, k)                                 # row for row
            assert np.abs(p - pp).max(initial=0.0) <= tol, (thr, k, np.abs(p - pp).max(initial=0.0))
        assert sum(len(c[0]) for c in closing) > 0
    closing, two, _ = eng.loop_posteriors(x, 0.0)
    helices = eng.helix_posteriors(x, 0.0, 2, 2)
    ctx = eng.context_profiles(x)
    for k, s in enumerate(seqs):
        L = len(s)
        cols, P = lc.dense_from_closing(L, closing[k])
        h2 = np.zeros((L, L + 1))
        h2[helices[k][0], helices[k][1]] = helices[k][3]
        lc.assert_identities(L, cols, P, lc.two_dict(two[k]), h2, ctx[k], tol, what=(opts, k))
    assert max(c[3][:, lc.S_].max() for c in closing) > 0.05


# ---- the loops of caller-given structures

def test_loops_of_structures_and_the_exact_zeros():
    """the MEA structure's loops against the table definition; a bulge or interior entry is bit-equal to the two-loop list entry
    of the same call; a pair that is no kept cell, a span above max_span and a two-loop that is no item give 0 exactly"""
    seqs, quals = batch((60, 33), seed=9, n_every=0, neg_every=0)
    base = engine_with(P1, 20)
    base.load_batch(seqs, quals)
    x = lc.loop_params(base)
    refs = cached("structs", lambda: table_refs(oracle_with(P1, x, 20), seqs, quals, x))
    kept = [np.zeros((len(s), len(s) + 1), dtype=bool) for s in seqs]
    for k, (ii, jj, _, _) in enumerate(base.pair_posteriors(x, 0.0)):
        kept[k][ii, jj] = True
    far = "(" + "." * 58 + ")"                                        # a span above max_span
    a, b = next((i, j) for i in range(33) for j in range(i + 6, 33) if not kept[1][i, j + 1])
    near = "".join("(" if p == a else ")" if p == b else "." for p in range(33))      # a cell the filter did not keep
    # a two-loop of kept cells: the best entry of the full list of sequence 0, as a structure of two pairs
    _, two, _ = base.loop_posteriors(x, 0.0)
    t = int(np.argmax(two[0][4]))
    i, j, k, l = (int(two[0][c][t]) for c in range(4))
    db = ["."] * 60
    db[i], db[j - 1], db[k], db[l - 1] = "(", ")", "(", ")"
    # a two-loop the inside enumeration does not hold: a kept outer cell around an inner cell the filter did not keep (at W = 20
    # every kept inner cell is an item: u1 + u2 <= 13 = C)
    listed = {(int(c), int(d), int(e), int(f)) for c, d, e, f in zip(*two[0][:4])}
    oi, oj, ik, il = next((oi, oj, ik, il) for oi in range(60) for oj in range(oi + 12, 61) if kept[0][oi, oj]
                          for ik in range(oi + 2, oj - 7) for il in range(ik + 5, oj - 1)
                          if not kept[0][ik, il] and (oi, oj, ik, il) not in listed)
    no_item = ["."] * 60
    no_item[oi], no_item[oj - 1], no_item[ik], no_item[il - 1] = "(", ")", "(", ")"
    mea = base.mea_structures(x, 1.0)[0]
    for opts in ((), PIPELINE3):
        eng = engine_with(P1, 20, opts)
        eng.load_batch(seqs, quals)
        _, _, _, loops = eng.loop_posteriors(x, np.inf, structures=[far, near])
        assert [tuple(int(v[0]) for v in lp[:3]) for lp in loops] == [(1, 0, 60), (1, a, b + 1)]
        assert loops[0][5][0] == 0.0 and loops[1][5][0] == 0.0 and not np.signbit(loops[0][5][0])
        _, two_e, _, loops = eng.loop_posteriors(x, 0.0, structures=["".join(db), mea[1]])
        lt, li, lj, lk, ll, lp = loops[0]
        assert (int(lt[0]) in (3, 4)) and (int(li[0]), int(lj[0]), int(lk[0]), int(ll[0])) == (i, j, k, l)
        sel = (two_e[0][0] == i) & (two_e[0][1] == j) & (two_e[0][2] == k) & (two_e[0][3] == l)
        assert sel.sum() == 1 and lp[0] == two_e[0][4][sel][0] > 0.0                       # bit for bit
        lt, li, lj, lk, ll, lp = loops[1]
        want = [refs[1][1].get((c, d, e, f), 0.0) if t_ in (3, 4) else refs[1][0][c, d, t_ - 1] for t_, c, d, e, f in zip(lt, li, lj, lk, ll)]
        lc.assert_loop(lp, want, what=("MEA loops", opts))
        loops = eng.loop_posteriors(x, np.inf, structures=["".join(no_item), "." * 33])[3]
        assert list(loops[0][5][:1]) == [0.0] and int(loops[0][0][0]) in (3, 4)


# ---- groupings, streamed batches, thresholds, and what a call leaves alone

def test_groupings_thresholds_and_what_a_call_leaves_alone():
    seqs, quals = nine()
    base = engine_with(P1, 50)
    base.load_batch(seqs, quals)
    x = lc.loop_params(base)
    lib = api.load_library()
    i32, dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    first = base.pair_posteriors(x, 0.0)
    helix = base.helix_posteriors(x, 0.0, 1, 8)
    cond = base.conditional_pairs(x, 1e-3, 1.0)
    _, stem = base.stem_profiles(x, 0.0)
    structs = base.mea_structures(x, 1.0)[0]
    first = base.pair_posteriors(x, 0.0)
    want_c, want_t, want_n, want_l = base.loop_posteriors(x, 0.0, structures=structs)
    n_c, n_t = sum(len(r[2]) for r in want_c), sum(len(r[4]) for r in want_t)
    assert n_c > 0 and n_t > 0 and sum(len(r[5]) for r in want_l) > 9
    # the lists of the last pair, conditional, stem and helix call are still those calls'
    n_cond = sum(len(r["i"]) for r in cond)
    qs, qi, qj = (np.full(n_cond, -1, dtype=np.int32) for _ in range(3))
    qm, qn = np.full(n_cond, np.nan), np.full(n_cond, np.nan)
    assert lib.elemdp_pair_conditional_list(base._h, qs.ctypes.data_as(i32), qi.ctypes.data_as(i32), qj.ctypes.data_as(i32),
                                            qm.ctypes.data_as(dp), qn.ctypes.data_as(dp), n_cond) == 0
    assert n_cond > 0 and np.array_equal(qi, np.concatenate([r["i"] for r in cond])) and np.array_equal(qm, np.concatenate([r["p_motif"] for r in cond]))
    n_stem = sum(len(r[3]) for r in stem)
    ss, si, sj, sk = (np.full(n_stem, -1, dtype=np.int32) for _ in range(4))
    sq = np.full(n_stem, np.nan)
    assert lib.elemdp_stem_list(base._h, ss.ctypes.data_as(i32), si.ctypes.data_as(i32), sj.ctypes.data_as(i32), sk.ctypes.data_as(i32),
                                sq.ctypes.data_as(dp), n_stem) == 0
    assert n_stem > 0 and np.array_equal(sk, np.concatenate([r[2] for r in stem])) and np.array_equal(sq, np.concatenate([r[3] for r in stem]))
    again = base._pair_lists(sum(len(r[0]) for r in first), np.concatenate([r[3] for r in first]))
    for a, b in zip(first, again):
        assert all(np.array_equal(u, v) for u, v in zip(a, b))
    n_hel = sum(len(r[3]) for r in helix)
    hcols = [np.full(n_hel, -1, dtype=np.int32) for _ in range(4)]
    hp = np.full(n_hel, np.nan)
    assert lib.elemdp_helix_list(base._h, *[c.ctypes.data_as(i32) for c in hcols], hp.ctypes.data_as(dp), n_hel) == 0
    assert n_hel > 0 and np.array_equal(hp, np.concatenate([r[3] for r in helix]))
    # and the loop lists survive theirs, bit for bit
    base.pair_posteriors(x, 0.5)
    base.helix_posteriors(x, 0.5)
    base.stem_profiles(x, 0.5)
    base.conditional_pairs(x, 0.5, 1.0)
    assert lib.elemdp_loop_closing_list(base._h, None, None, None, None, None, n_c - 1) == -1     # (its length too)
    assert lib.elemdp_loop_two_list(base._h, None, None, None, None, None, None, n_t - 1) == -1
    cs, ci, cj = (np.full(n_c, -1, dtype=np.int32) for _ in range(3))
    cp, cc_ = np.full(n_c, np.nan), np.full((n_c, 5), np.nan)
    assert lib.elemdp_loop_closing_list(base._h, cs.ctypes.data_as(i32), ci.ctypes.data_as(i32), cj.ctypes.data_as(i32),
                                        cp.ctypes.data_as(dp), cc_.ctypes.data_as(dp), n_c) == 0
    assert np.array_equal(cs, np.concatenate([np.full(len(r[2]), k, dtype=np.int32) for k, r in enumerate(want_c)]))
    assert np.array_equal(cp, np.concatenate([r[2] for r in want_c])) and np.array_equal(cc_, np.concatenate([r[3] for r in want_c]))
    tcols = [np.full(n_t, -1, dtype=np.int32) for _ in range(5)]
    tp = np.full(n_t, np.nan)
    assert lib.elemdp_loop_two_list(base._h, *[c.ctypes.data_as(i32) for c in tcols], tp.ctypes.data_as(dp), n_t) == 0
    assert np.array_equal(tp, np.concatenate([r[4] for r in want_t])) and np.array_equal(tcols[3], np.concatenate([r[2] for r in want_t]))
    # a finite threshold keeps exactly the entries of the full lists at or above it, in order; the counts do not move.  (The values
    # of two calls are equal to rounding, as across groupings below: the sum passes of two calls do not give the same bits.)
    for thr in (1e-3, 0.3):
        got_c, got_t, got_n = base.loop_posteriors(x, thr)
        for a, b in zip(got_c, want_c):
            assert np.abs(b[2] - thr).min(initial=1.0) > 1e-9                # (no entry of this batch lies within rounding of the threshold)
            keep = b[2] >= thr
            assert all(np.array_equal(u, v[keep]) for u, v in zip(a[:2], b[:2]))
            for u, v in zip(a[2:], b[2:]):
                np.testing.assert_allclose(u, v[keep], rtol=1e-10, atol=1e-14)
        for a, b in zip(got_t, want_t):
            assert np.abs(b[4] - thr).min(initial=1.0) > 1e-9
            keep = b[4] >= thr
            assert all(np.array_equal(u, v[keep]) for u, v in zip(a[:4], b[:4]))
            np.testing.assert_allclose(a[4], b[4][keep], rtol=1e-10, atol=1e-14)
        np.testing.assert_allclose(got_n, want_n, rtol=1e-10, atol=1e-14)
        assert 0 < sum(len(a[2]) for a in got_c) < n_c and 0 < sum(len(a[4]) for a in got_t) < n_t
    # without the counts only the cells whose P reaches the threshold are walked: the same lists
    mc, mt = C.c_int64(), C.c_int64()
    assert lib.elemdp_loop_posteriors(base._h, np.ascontiguousarray(x).ctypes.data_as(dp), base.n_param, 0.3, None, C.byref(mc),
                                      C.byref(mt), None, None, None) == 0
    assert (mc.value, mt.value) == (sum(len(a[2]) for a in got_c), sum(len(a[4]) for a in got_t))
    tp2 = np.full(mt.value, np.nan)
    assert lib.elemdp_loop_two_list(base._h, None, None, None, None, None, tp2.ctypes.data_as(dp), mt.value) == 0
    np.testing.assert_allclose(tp2, np.concatenate([a[4] for a in got_t]), rtol=1e-10, atol=1e-14)
    # the pruned call in both forms: its lists are the cut of the full lists, columns included, and a cell below the bound is not
    # listed through its two-loops either
    for opts in ((), PIPELINE3):
        eng = engine_with(P1, 50, opts)
        eng.load_batch(seqs, quals)
        cut_c, cut_t, none = eng.loop_posteriors(x, 0.3, counts=False)
        assert none is None
        for k, (a, b) in enumerate(zip(cut_c, want_c)):
            keep = b[2] >= 0.3
            assert all(np.array_equal(u, v[keep]) for u, v in zip(a[:2], b[:2])), (opts, k)
            for u, v in zip(a[2:], b[2:]):
                np.testing.assert_allclose(u, v[keep], rtol=1e-8, atol=1e-10, err_msg=str((opts, k)))
        for k, (a, b) in enumerate(zip(cut_t, want_t)):
            keep = b[4] >= 0.3
            assert all(np.array_equal(u, v[keep]) for u, v in zip(a[:4], b[:4])), (opts, k)
            np.testing.assert_allclose(a[4], b[4][keep], rtol=1e-8, atol=1e-10, err_msg=str((opts, k)))
        assert sum(len(a[3]) for a in cut_c) > 0 and max(a[3][:, [lc.B_, lc.I_]].max(initial=0.0) for a in cut_c) > 0.01
    lists = base.loop_posteriors(x, np.inf)
    assert all(len(c[2]) == 0 for c in lists[0]) and all(len(t[4]) == 0 for t in lists[1]) and np.allclose(lists[2], want_n, rtol=1e-10, atol=1e-14)
    for opts in ((("group", 1),), (("group", 3),), (("max_resident", 4),), (("poison", 1),)):
        eng = engine_with(P1, 50, opts)
        eng.load_batch(seqs, quals)
        got_c, got_t, got_n, got_l = eng.loop_posteriors(x, 0.0, structures=structs)
        for k in range(len(seqs)):
            assert all(np.array_equal(u, v) for u, v in zip(got_c[k][:2], want_c[k][:2])), (opts, k)
            assert all(np.array_equal(u, v) for u, v in zip(got_t[k][:4], want_t[k][:4])), (opts, k)
            assert all(np.array_equal(u, v) for u, v in zip(got_l[k][:5], want_l[k][:5])), (opts, k)
            for g, w in ((got_c[k][2], want_c[k][2]), (got_c[k][3], want_c[k][3]), (got_t[k][4], want_t[k][4]), (got_l[k][5], want_l[k][5])):
                np.testing.assert_allclose(g, w, rtol=1e-10, atol=1e-14, err_msg=str((opts, k)))
        np.testing.assert_allclose(got_n, want_n, rtol=1e-10, atol=1e-14)


def test_a_streamed_call_without_lists_leaves_two_empty_lists():
    """Two sequences that stream as two chunks (max_resident 1), min_prob +inf after a call with min_prob 0: the chunks keep no
    lists, and the handle's lists are empty, with count 0 and not the -1 of 'no list'; the loops of the structures are those of the
    first call.  Bit for bit in the log-space form (pipeline 3), whose sums have a fixed order.  The sum passes of the scaled-linear
    form add with floating-point atomics, so two calls of it agree to rounding only, as with the thresholds and groupings above
    (seen here: 5 of 6 probabilities of one sequence 2.2e-16 apart between two identical calls, none of the other's); there the
    probabilities are held to that test's rtol 1e-10."""
    lib = api.load_library()
    dp = C.POINTER(C.c_double)
    seqs, quals = batch((40, 37), seed=5, n_every=0, neg_every=0)
    off = np.concatenate([[0], np.cumsum([len(s) for s in seqs])])
    for opts in (PIPELINE3, ()):
        eng = engine_with(P1, 50, opts + (("max_resident", 1),))
        eng.load_batch(seqs, quals)
        x = lc.loop_params(eng)
        structs = eng.mea_structures(x, 1.0)[0]
        first = eng.loop_posteriors(x, 0.0, structures=structs)
        assert sum(len(r[2]) for r in first[0]) > 0 and sum(len(r[4]) for r in first[1]) > 0 and sum(len(r[5]) for r in first[3]) > 2
        got = eng.loop_posteriors(x, np.inf, structures=structs)
        assert all(len(c[2]) == 0 for c in got[0]) and all(len(t[4]) == 0 for t in got[1])
        # the counts of the lists and their fetches, past the wrapper: 0 entries, not "no list"
        ltype, lprob, counts = np.full(off[-1], -1, dtype=np.int32), np.full(off[-1], -1.0), np.zeros((2, 5))
        mc, mt = C.c_int64(-7), C.c_int64(-7)
        assert lib.elemdp_loop_posteriors(eng._h, np.ascontiguousarray(x).ctypes.data_as(dp), eng.n_param, np.inf, counts.ctypes.data_as(dp),
                                          C.byref(mc), C.byref(mt), "".join(structs).encode(), ltype.ctypes.data_as(C.POINTER(C.c_int32)),
                                          lprob.ctypes.data_as(dp)) == 0
        assert (mc.value, mt.value) == (0, 0)
        assert lib.elemdp_loop_closing_list(eng._h, None, None, None, None, None, 0) == 0       # (-4, ELEMDP_ESTATE, without lists)
        assert lib.elemdp_loop_two_list(eng._h, None, None, None, None, None, None, 0) == 0
        for k, (a, b) in enumerate(zip(got[3], first[3])):
            p = b[5]
            for what, q in (("wrapper", a[5]), ("library", lprob[off[k] + b[1]])):
                print("%s, sequence %d, %s: loop_prob differs from the first call's in %d of %d, by at most %.3g"
                      % (opts, k, what, (q != p).sum(), len(p), np.abs(q - p).max()))
            assert np.array_equal(ltype[off[k] + b[1]], b[0]) and all(np.array_equal(u, v) for u, v in zip(a[:5], b[:5]))
            if opts == PIPELINE3:
                assert np.array_equal(a[5], p) and np.array_equal(lprob[off[k] + b[1]], p)
            else:
                np.testing.assert_allclose(a[5], p, rtol=1e-10, atol=1e-14)
                np.testing.assert_allclose(lprob[off[k] + b[1]], p, rtol=1e-10, atol=1e-14)


def test_refusals():
    lib = api.load_library()
    dp = C.POINTER(C.c_double)
    eng = engine_with(P1, 50)
    x = lc.loop_params(eng)
    xp = np.ascontiguousarray(x).ctypes.data_as(dp)
    assert lib.elemdp_loop_posteriors(eng._h, xp, eng.n_param, 0.0, None, None, None, None, None, None) == -4        # ELEMDP_ESTATE
    seqs, quals = batch((30,), seed=3, n_every=0, neg_every=0)
    eng.load_batch(seqs, quals)
    assert lib.elemdp_loop_closing_list(eng._h, None, None, None, None, None, 0) == -4
    assert lib.elemdp_loop_two_list(eng._h, None, None, None, None, None, None, 0) == -4
    lt = np.zeros(30, dtype=np.int32)
    ltp = lt.ctypes.data_as(C.POINTER(C.c_int32))
    for args in ((None, 0.0, None, None), (xp, -1.0, None, None), (xp, np.nan, None, None), (xp, 0.0, ("(" * 30).encode(), ltp),
                 (xp, 0.0, ("x" * 30).encode(), ltp), (xp, 0.0, ("." * 30).encode(), None)):
        assert lib.elemdp_loop_posteriors(eng._h, args[0], eng.n_param, args[1], None, None, None, args[2], args[3], None) == -1, args
    assert lib.elemdp_loop_posteriors(eng._h, xp, eng.n_param + 1, 0.0, None, None, None, None, None, None) == -1
    assert lib.elemdp_loop_posteriors(eng._h, xp, eng.n_param, 0.0, None, None, None, None, None, None) == 0
    assert lib.elemdp_loop_closing_list(eng._h, None, None, None, None, None, 1 << 20) == 0


# ---- command line

def test_command_line_writes_the_loop_files(tmp_path):
    fq, model = gpath("positive_head6.fq"), gpath("trna_a.model")
    a1, lf, mf = str(tmp_path / "a.raw"), str(tmp_path / "loops.txt"), str(tmp_path / "mea_loops.txt")
    cli.main(["scan", "-f", fq, "-q", model, "--out1", a1, "--out-loops", lf, "--loop-min-prob", "0.05", "--out-mea-loops", mf,
              "--mea-gamma", "2"])
    recs = io.read_fastq(fq)
    m = io.read_model(model)
    eng = io.engine_from_model(m)
    eng.load_batch([s for _, s, _ in recs], [q for _, _, q in recs])
    structs, _, pairs = eng.mea_structures(m["x"], 2.0, 0.0)
    closing, two, _, loops = eng.loop_posteriors(m["x"], 0.05, structures=structs, counts=False)      # (as the command line calls it)
    got = io.read_loops(lf)
    assert "".join(io.loop_line(r["id"], r["type"], r["i"] + 1, r["j"], None if r["k"] is None else r["k"] + 1, r["l"], r["p"])
                   for r in got) == open(lf).read()
    want = "".join(io.loop_lines(rid, c, t) for (rid, _, _), c, t in zip(recs, closing, two))
    assert want == open(lf).read() and len(got) > 0 and {r["type"] for r in got} >= {"H", "S"}
    n_two = sum(len(t[4]) for t in two)
    assert sum(r["type"] in "BI" for r in got) == n_two
    got = io.read_mea_loops(mf)
    want = [(rid, api.LOOP_TYPES[t], int(i), int(j), p) for (rid, _, _), lp in zip(recs, loops) for t, i, j, _, _, p in zip(*lp)]
    assert len(got) == len(want) > 0
    have = [{(int(a), int(b)): float(v) for a, b, v in zip(pr[0], pr[1], pr[2])} for pr in pairs]
    ids = [rid for rid, _, _ in recs]
    for g, w in zip(got, want):
        assert (g["id"], g["type"], g["i"], g["j"]) == w[:4] and g["p"] == pytest.approx(w[4], rel=1e-5, abs=1e-12)
        assert g["p_pair"] == pytest.approx(have[ids.index(g["id"])][(g["i"], g["j"])], rel=1e-5)
        assert g["p"] <= g["p_pair"] * (1 + 1e-5) + 1e-12
