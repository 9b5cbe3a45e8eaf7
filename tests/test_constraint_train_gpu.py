"""The train evaluation under hard structure constraints against the oracle, sequence by sequence: the
seq_stats row and the count columns ENo, ENx, EHo, EHx that the outside pass of the train schedule (k4_out, the loop outside
kernels, the L chain, k4_combine / k3_combine) and k_reduce produce, which test_constraint_gpu.py compares with nothing.

a. the enumerated cases against the enumeration reference of tests/constraint_train_check.py (justified without a GPU in
   tests/test_constraint_train_cpu.py), under every option that changes the train kernels or their schedule;
b. a whole structure given back as the string at L 47 to 107 and 64 to 128 states, against the oracle's train row of that one
   structure;
c. the partition identity of the counts, Z X = Z_x X_x + Z_| X_| and Z_| X_| = Z_< X_< + Z_> X_>, up to L 257;
d. a streamed batch and a window of evaluation over constrained sequences.

Every reference comes from the oracle alone."""
import threading
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from oracle import pyoracle as po
from rnaelem_amd import api, synth
from tests import constraint_check as kc
from tests import constraint_train_check as kt
from tests import ctx_check as cc
from tests import joint_check as jc
from tests import large_automata as la
from tests import train_check as tc
from tests.pair_check import n_workers, oracle_pairs, unpaired_of
from tests.test_constraint_gpu import BIG, P1, PAR, SWITCHES, whole_inputs, with_chars
from tests.test_pair_posterior_gpu import perturbed
from tests.util import assert_log_close

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cases():
    return kt.train_cases()


def engine(pattern, W, min_bpp, flags, opts):
    eng = api.Engine(pattern, PAR, W, 30, min_bpp, 0.1, flags, 0)
    for key, v in opts:
        eng.set_option(key, v)
    return eng


# ---- a. the enumerated cases

A_OPTS = {
    "default": (), "fast0": (("fast", 0),), "schedule0": (("schedule", 0),), "deterministic": (("deterministic", 1),),
    "pipeline3": (("pipeline", 3),), "poison": (("poison", 1),), "group1": (("group", 1),), "group3": (("group", 3),),
    "lik-ratio": (),
}
A_OPTS.update({key + "0": ((key, 0),) for key in SWITCHES})


@pytest.mark.parametrize("name", list(A_OPTS))
def test_enumerated_cases_rows_and_sums(name, cases):
    """Per case one batch: under each label a free copy and every string.  The rows with all four vectors go through
    check_train_path (rows, fn, gr, sum_eff, n_skipped and the count segments of train_partial against the sums over the reference
    rows; train_finish; a repeated evaluation); the strings whose Zo- and Znasi-weighted vectors have no route are evaluated in a
    batch of their own, for Z, f, skipped and the vectors they have.  An unsatisfiable string and a string that leaves no parse
    with the motif are skipped with count columns of exactly 0 (check_rows) among live neighbours.  lik-ratio: the first quoted
    case, whose reference test_constraint_train_cpu.py holds under LIK_RATIO too."""
    opts = A_OPTS[name]
    n_skipped = n_partial = 0
    for case, x, s, q, refs, _ in cases:
        pattern, L, flags, min_bpp = case
        if name == "lik-ratio":
            if case != kc.QUOTED[0][0]:
                continue
            flags |= api.LIK_RATIO
        (seqs, quals, cons, rows), (seqs_p, quals_p, cons_p, rows_p) = kt.batch_of(case, x, s, q, refs, flags=flags)
        assert len(seqs) >= 4 and cons[0] is None
        eng = engine(pattern, 50, min_bpp, flags, opts)
        eng.load_batch(seqs, quals, constraints=cons)
        trefs = kt.train_refs(rows, len(x))
        _, res, stats, counts = tc.check_train_path(eng, seqs, quals, x, None, refs=trefs)
        n_skipped += res[3]
        if name == "deterministic":         # bit for bit from one evaluation to the next
            res2 = eng.train_eval(x)
            c2 = eng.seq_counts()
            assert res2[0] == res[0] and np.array_equal(res2[1], res[1]), case
            assert np.array_equal(eng.seq_stats(), stats, equal_nan=True), case
            assert all(np.array_equal(c2[key], counts[key]) for key in tc.COUNTS), case
        if seqs_p:
            eng.load_batch(seqs_p, quals_p, constraints=cons_p)
            eng.train_eval(x)
            n_partial += kt.check_partial_rows(eng.seq_stats(), eng.seq_counts(), rows_p, seqs_p, quals_p)
    assert name == "lik-ratio" or (n_skipped >= 2 and n_partial >= 4)          # (the quoted case has neither)


def test_no_parse_conventions_under_a_constraint(cases):
    """`..........|.........` has no structure; all-x under `(.*)` leaves Z(nasi) finite and Z(ari) = -inf.  Both are skipped,
    their four count columns are exactly 0, and gr and the partial vector of the batch are those of the batch without them."""
    case, x, s, q, refs, _ = cases[len(jc.CASES) + 1]
    pattern, L, flags, min_bpp = case
    assert pattern == "(.*)" and [c for c, e in refs if not np.isfinite(e["lnZ"])] == ["..........|........."]
    keep = [(c, e) for c, e in refs if np.isfinite(e["lnZ"])]
    (seqs, quals, cons, rows), _ = kt.batch_of(case, x, s, q, keep, flags=flags)
    base = engine(pattern, 50, min_bpp, flags, ())
    base.load_batch(seqs, quals, constraints=cons)
    res0 = base.train_eval(x)
    part0 = base.train_partial(x)
    extra = ["x" * L, "..........|.........", "x" * L]
    where = (1, len(seqs) // 2, len(seqs))          # among the live ones, under both labels
    s2, q2, c2 = list(seqs), list(quals), list(cons)
    for at, c in sorted(zip(where, extra), reverse=True):
        s2.insert(at, s)
        q2.insert(at, quals[min(at, len(quals) - 1)])
        c2.insert(at, c)
    eng = engine(pattern, 50, min_bpp, flags, ())
    eng.load_batch(s2, q2, constraints=c2)
    res = eng.train_eval(x)
    st, cn = eng.seq_stats(), eng.seq_counts()
    part = eng.train_partial(x)
    o = kt.case_oracle(case, flags, x)
    for k, c in enumerate(c2):
        if c in extra:
            assert st[k, 4] == 1 and all(np.all(cn[key][k] == 0.0) for key in tc.COUNTS), (k, c)
            if c == "x" * L:          # one structure, without a pair: its weight is all Z(nasi)
                assert np.isneginf(st[k, 1]), st[k]
                assert_log_close(st[k, [0, 2]], [o.derivation_logz(s, q2[k], "." * L, None)] * 2, what="all-x")
            else:
                assert np.all(np.isneginf(st[k, :3])), st[k]
    assert res[3] == res0[3] + 3 and res[2] == pytest.approx(res0[2], rel=1e-12) and res[0] == pytest.approx(res0[0], rel=1e-12)
    np.testing.assert_allclose(res[1], res0[1], rtol=1e-11, atol=1e-12)
    np.testing.assert_allclose(part[4:], part0[4:], rtol=1e-11, atol=1e-12)
    assert part[0] == pytest.approx(part0[0], rel=1e-12) and part[3] == part0[3] + 3


# ---- b. a whole structure at real sizes

B_CASES = ["L47", "L107", "S64", "S126", "S128"]
_whole = {}


def whole_case(which):
    """pattern, W, x, seq, [qual per label], [the oracle's row of the one structure per label], the string"""
    if which in _whole:
        return _whole[which]
    if which in ("S126", "S128"):          # the planted sequences of large_automata.scan_batch, the shortest first
        S = int(which[1:])
        pattern, W = la.PATTERN[S], 50
        every = 1 if S == 128 else 2
        cands = [(s, q) for k, (s, q) in enumerate(zip(*la.scan_batch(S))) if k % every == 0]
        x = perturbed(api.Engine(pattern, PAR, W, 30, 1e-4, 0.1, 0, 0))
        o = cc.ctx_oracle(pattern, W, 30, min_bpp=1e-4)
        o.set_params(x)
    else:
        pattern, W, x, s, q, o = whole_inputs(which)
        cands = [(s, q)]
    free = api.Engine(pattern, PAR, W, 30, 1e-4, 0.1, 0, 0)
    if which[0] == "S":
        assert free.n_state == int(which[1:])
    of = cc.ctx_oracle(pattern, W, 30, min_bpp=1e-4, flags=po.DBG_FIX_RSS)
    of.set_params(x)
    db = None
    for s, q in cands:
        free.load_batch([s], [q])
        # the MEA structure; where it has no parse with the motif, the CYK structure of the scan, which is one
        for cand in (free.mea_structures(x, 1.0)[0][0], kc.letters_to_db(free.scan(x)[0][0]["rss"])):
            if "(" in cand and not of.train_seq(s, kt.labelled(q, 0), fix_rss=cand)["skipped"]:
                db = cand
                break
        if db is not None:
            break
    assert db is not None, which
    quals = [kt.labelled(q, last) for last in kt.LABELS]
    rows = []
    for ql in quals:
        r = of.train_seq(s, ql, fix_rss=db)
        del r["inside_o"], r["outside_o"]
        assert not r["skipped"] and np.isfinite(r["Zari"]), which          # the structure has a parse with the motif
        r["bpp_eff"] = o.bpp(s)[2]          # (the filter sees no constraint)
        rows.append(r)
    _whole[which] = (pattern, W, x, s, quals, rows, db.replace(".", "x"))
    return _whole[which]


@pytest.mark.parametrize("opts", [(), (("schedule", 0),), (("pipeline", 3),)], ids=["default", "schedule0", "pipeline3"])
@pytest.mark.parametrize("which", B_CASES)
def test_train_row_of_a_whole_structure(which, opts):
    """the structure of the free fold as a string of ( ) and x: the ensemble is that one structure, and the whole train row under
    both labels is the DBG_FIX_RSS oracle's train_seq(fix_rss=db)"""
    pattern, W, x, s, quals, rows, cons = whole_case(which)
    eng = engine(pattern, W, 1e-4, 0, opts)
    eng.load_batch([s] * 2, quals, constraints=[cons] * 2)
    tc.check_train_path(eng, [s] * 2, quals, x, None, refs=kt.train_refs(rows, len(x)))


# ---- c. the partition identity of the counts

C_SHAPES = [(47, 20, BIG[0][2]), (107, 50, BIG[1][2]), (131, 50, 1131), (257, 100, 1257)]          # (L, max_span, synth seed)
_identity = {}


def identity_inputs(L, W, seed):
    """x, seq, qual, the base p whose unpaired probability u by the oracle is nearest 1/2, u, the free oracle's rows per label"""
    if (L, W) not in _identity:
        (s,), (q,) = synth.synth_batch(1, L, seed=seed)
        x = perturbed(api.Engine(P1, PAR, W, 30, 1e-4, 0.1, 0, 0))
        local = threading.local()

        def job(last):
            local.o = cc.ctx_oracle(P1, W, 30, min_bpp=1e-4)
            local.o.set_params(x)
            if last is None:
                return oracle_pairs(local.o, s, q)
            r = local.o.train_seq(s, kt.labelled(q, last))
            del r["inside_o"], r["outside_o"]
            return r

        with ThreadPoolExecutor(max_workers=min(3, n_workers())) as ex:
            P, r0, r5 = ex.map(job, [None] + list(kt.LABELS))
        u = unpaired_of(P, L)
        p = int(np.argmin(np.abs(u - 0.5)))
        assert 0.05 <= u[p] <= 0.95, u[p]
        _identity[(L, W)] = (x, s, q, p, u[p], [r0, r5])
    return _identity[(L, W)]


@pytest.mark.parametrize("opts", [(), (("pipeline", 3),)], ids=["default", "pipeline3"])
@pytest.mark.parametrize("L,W,seed", C_SHAPES, ids=["L47", "L107", "L131", "L257"])
def test_partition_identity_of_the_counts(L, W, seed, opts):
    """One sequence under both labels, free and with x, |, < and > on one base.  Per count vector X with the Z of its ensemble (Zo
    for ENo and EHo, Zari for ENx and EHx with the motif, Znasi without; read from seq_stats), in units of the free Z:
    X = a_x X_x + a_| X_| and a_| X_| = a_< X_< + a_> X_>, a_c = exp(Z_c - Z).  Three terms each within the project's per-row bound:
    rtol 1e-8, atol 3 ROW_ATOL (the rule of test_partition_identity_of_the_outside_based_products)."""
    x, s, q, p, u, free_rows = identity_inputs(L, W, seed)
    chars = (None, "x", "|", "<", ">")
    seqs, quals, cons = [], [], []
    for last in kt.LABELS:
        for ch in chars:
            seqs.append(s)
            quals.append(kt.labelled(q, last))
            cons.append(None if ch is None else with_chars(L, {p: ch}))
    eng = engine(P1, W, 1e-4, 0, opts)
    eng.load_batch(seqs, quals, constraints=cons)
    eng.train_eval(x)
    st, cn = eng.seq_stats(), eng.seq_counts()
    n = len(chars)
    for lab, last in enumerate(kt.LABELS):
        k0 = lab * n
        # the free copy against the oracle's row
        rows = [None] * len(seqs)
        rows[k0] = free_rows[lab]
        tc.check_rows(st, cn, tc.TrainRefs(rows, None), seqs, quals, first=k0, count=1)
        # the weights of x and | in the whole ensemble against the oracle's unpaired probability
        assert abs(np.exp(st[k0 + 1, 0] - st[k0, 0]) - u) <= 2e-9 and abs(np.exp(st[k0 + 2, 0] - st[k0, 0]) - (1.0 - u)) <= 2e-9, (L, last)
        for k in range(k0, k0 + n):          # a copy with a parse is not skipped: its columns are counts, not zeros
            assert st[k, 4] == 0 or np.isneginf(st[k, 0]), (L, last, chars[k - k0], st[k])
        assert st[k0 + 1, 4] == 0 and st[k0 + 2, 4] == 0
        zcol = {"ENo": 0, "EHo": 0, "ENx": 1 if last == 0 else 2, "EHx": 1 if last == 0 else 2}
        for key in tc.COUNTS:
            z = st[k0:k0 + n, zcol[key]]
            a = np.exp(z - z[0])          # (exp(-inf) = 0: a copy without a parse)
            X = cn[key][k0:k0 + n]
            what = "L %d %s %s" % (L, tc.label(quals[k0]), key)
            np.testing.assert_allclose(a[1] * X[1] + a[2] * X[2], X[0], rtol=1e-8, atol=3 * tc.ROW_ATOL, err_msg=what + ": x and |")
            np.testing.assert_allclose(a[3] * X[3] + a[4] * X[4], a[2] * X[2], rtol=1e-8, atol=3 * tc.ROW_ATOL, err_msg=what + ": < and >")
            # (the two conditioned rows are two different things wherever the motif's emissions count; without the motif every
            # base is emitted by the background whatever the structure, and ENx is the same vector in all five copies)
            if key == "ENo" or (key == "ENx" and last == 0):
                assert np.abs(X[1] - X[2]).max() > 1e-6, what


# ---- d. batch plumbing

def plumbing_batch(cases):
    """the enumerated case the engine of c serves (`((.*.))`, flags 0, min_bpp 1e-4, at max_span 50: its complete rows), then the
    four sequences of c with | or x on the base of c"""
    case, x, s, q, refs, _ = cases[1]          # (x: the case's own parameters, at which its reference rows are)
    assert case == (P1, 14, 0, 1e-4)
    seqs, quals, cons = [], [], []
    for k, (L, W, seed) in enumerate(C_SHAPES):
        _, s_k, q_k, p, _, _ = identity_inputs(L, W, seed)
        seqs.append(s_k)
        quals.append(kt.labelled(q_k, kt.LABELS[k % 2]))
        cons.append(with_chars(L, {p: "|x"[k % 2]}))
    return case, x, s, q, refs, seqs, quals, cons


def test_streamed_constrained_batch_equals_the_resident_one(cases):
    case, x, s, q, refs, seqs, quals, cons = plumbing_batch(cases)
    (es, eq, ec, _), (ps, pq, pc, _) = kt.batch_of(case, x, s, q, refs)
    seqs, quals, cons = es[:3] + seqs[:2] + es[3:] + ps + seqs[2:], eq[:3] + quals[:2] + eq[3:] + pq + quals[2:], ec[:3] + cons[:2] + ec[3:] + pc + cons[2:]
    res = engine(P1, 50, 1e-4, 0, ())
    res.load_batch(seqs, quals, constraints=cons)
    want = res.train_eval(x)
    st = res.seq_stats()
    assert all(st[k, 4] == 0 for k, c in enumerate(cons) if len(seqs[k]) > 40) and 0 < want[3] < len(seqs)
    eng = engine(P1, 50, 1e-4, 0, (("max_resident", 3),))
    eng.load_batch(seqs, quals, constraints=cons)
    for sweep in range(2):          # (the second from the mask cache)
        fn, gr, eff, nsk = eng.train_eval(x)
        assert nsk == want[3] and eff == pytest.approx(want[2], rel=1e-12), sweep
        assert abs(fn - want[0]) <= 1e-9 * max(1.0, abs(want[0])), (sweep, fn, want[0])
        np.testing.assert_allclose(gr, want[1], err_msg="sweep %d" % sweep, **tc.GR_TOL)
        assert_log_close(eng.seq_stats()[:, :3], st[:, :3], what="sweep %d" % sweep)


def test_a_window_inside_the_constrained_sequences(cases):
    """eval_first / eval_count from the second row of the enumerated part to its last but one (both constrained; the free copy of
    the second label lies inside), with the long constrained sequences of c in front and behind: the window's rows and sums
    against the enumeration reference, at the case's own parameters"""
    case, x, s, q, refs, seqs, quals, cons = plumbing_batch(cases)
    (es, eq, ec, rows), _ = kt.batch_of(case, x, s, q, refs)
    assert len(es) >= 4 and ec[1] is not None and ec[-2] is not None
    all_s, all_q, all_c = seqs[:2] + es + seqs[2:], quals[:2] + eq + quals[2:], cons[:2] + ec + cons[2:]
    eng = engine(P1, 50, 1e-4, 0, ())
    eng.load_batch(all_s, all_q, constraints=all_c)
    trefs = tc.TrainRefs([None] * 2 + rows + [None] * 2, None)          # (only the window's rows are read)
    res = kt.check_window(eng, x, trefs, all_s, all_q, 3, len(es) - 2)
    whole = eng.train_eval(x)
    assert np.abs(whole[1] - res[1]).max() > 1e-3          # (the window was a window)


def test_worst_count_error_seen():
    """(last: it reads what the cases above recorded)"""
    print("worst per-sequence count error under constraints |gpu - reference| / (%g + |reference|) = %.3e at %s" % (
        tc.ROW_ATOL / tc.ROW_RTOL, tc.WORST["err"], tc.WORST["where"]))
    assert tc.WORST["err"] <= tc.ROW_RTOL
