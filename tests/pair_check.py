"""Shared checks of the pair path (DESIGN.md sections 12 and 13): base-pair posteriors and unpaired probabilities against the
oracle's inside / outside tables, MEA structures against the host mirror (bit for bit, on the call's own posteriors) and against
the optimum over the oracle's posteriors, scan records against the oracle's scan.

The oracle work runs over the sequences of a batch in a thread pool (the oracle's C calls release the GIL), one oracle handle per
worker thread."""
import os
import threading
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from tests.mea_mirror import expected_accuracy, mea_fold, pair_matrix, pairs_of
from tests.util import assert_log_close

GAMMAS = (1e-3, 0.5, 1.0, 4.0, 1e3)     # the MEA weights of the full check; the optimum is checked at OPT_GAMMAS
OPT_GAMMAS = (1.0, 4.0)


def oracle_pairs(o, seq, qual, scan=None):
    """P[i, d] = sum_s exp(inside + outside - Z) over plane P of the train schedule's first (full-terminal) pass, or None for a
    sequence without any parse (Z(ari, nasi) = 0).  A sequence the train schedule skips for Z(ari) = 0 alone (no parse with the
    motif, motif_trainer.hpp:211-215) still has the pairs of its parses without the motif: the oracle runs that one outside pass
    for its tables.  scan: the oracle's scan record of the sequence when the caller has it already."""
    t = o.train_seq(seq, qual, tables=True)
    Zo = t["Zo"]
    if not np.isfinite(Zo):
        return None
    ZL = (scan if scan is not None else o.scan_seq(seq, qual))["ZL"]
    assert Zo == pytest.approx(ZL, rel=1e-12)
    with np.errstate(invalid="ignore"):
        P = np.exp(t["inside"][:, :, 0, :] + t["outside"][:, :, 0, :] - Zo).sum(axis=2)
    return np.nan_to_num(P, nan=0.0)


def unpaired_of(P, L):
    u = np.ones(L)
    W = P.shape[1] - 1
    for i in range(L + 1):
        for d in range(1, W + 1):
            if i + d <= L and P[i, d] != 0.0:
                u[i] -= P[i, d]
                u[i + d - 1] -= P[i, d]
    return u


def n_workers():
    return max(1, min(16, len(os.sched_getaffinity(0))))


def oracle_refs(make_oracle, seqs, quals):
    """Per sequence {"P": oracle_pairs (None: no parse), "scan": the oracle's scan record}, computed in parallel:
    make_oracle() returns a fresh oracle handle with the parameters set, one per worker thread."""
    local = threading.local()

    def one(k):
        if not hasattr(local, "o"):
            local.o = make_oracle()
        sc = local.o.scan_seq(seqs[k], quals[k])
        return dict(P=oracle_pairs(local.o, seqs[k], quals[k], scan=sc), scan=sc)

    order = sorted(range(len(seqs)), key=lambda k: -len(seqs[k]))     # (longest first: the pool drains evenly)
    with ThreadPoolExecutor(max_workers=n_workers()) as ex:
        done = dict(zip(order, ex.map(one, order)))
    return [done[k] for k in range(len(seqs))]


def check_pair_lists(eng, seqs, res, Ps):
    """res: pair_posteriors(x, 0.0); Ps: the oracle's P per sequence (None: no parse); eng: an engine with the batch resident
    (its kept cells).  The list holds exactly the kept cells in (i, j) order; P and unpaired match the oracle; a sequence the
    has no parse has P = 0 and unpaired = 1 exactly."""
    assert len(res) == len(seqs) == len(Ps)
    for k, (seq, P) in enumerate(zip(seqs, Ps)):
        L = len(seq)
        ii, jj, pp, unp = res[k]
        assert len(unp) == L, k
        kept, _ = eng.pairs(k)
        d = jj - ii
        ki, kd = np.nonzero(kept)
        sel = (kd >= 1) & (ki + kd <= L)
        assert list(zip(ii, d)) == list(zip(ki[sel], kd[sel])), k
        if P is None:
            assert np.all(pp == 0.0), ("sequence without a parse", k, pp[pp != 0.0][:5])
            assert np.all(unp == 1.0), ("sequence without a parse", k, unp[unp != 1.0][:5])
            continue
        np.testing.assert_allclose(pp, P[ii, d], rtol=1e-8, atol=1e-12, err_msg="sequence %d" % k)
        mask = np.zeros_like(P, dtype=bool)
        mask[ii, d] = True
        assert np.all(P[~mask] == 0.0), k          # nothing outside the filter's pairs
        np.testing.assert_allclose(unp, unpaired_of(P, L), rtol=1e-8, atol=1e-10, err_msg="unpaired %d" % k)


def check_against_oracle(eng, o, seqs, quals, x):
    """pair_posteriors(x, 0.0) against one oracle handle o (parameters set), sequence by sequence"""
    res = eng.pair_posteriors(x, 0.0)
    Ps = [oracle_pairs(o, s, q) for s, q in zip(seqs, quals)]
    check_pair_lists(eng, seqs, res, Ps)
    assert sum(P is not None for P in Ps) >= min(3, len(seqs))
    return res


def check_structure(eng, k, L, s):
    """balanced, of length L, and every pair a kept cell of span 2 .. W"""
    assert len(s) == L, k
    W = min(L, eng.max_span)
    kept = eng.pairs(k)[0]
    cells = pairs_of(s)
    assert all(2 <= d <= W and i + d <= L and kept[i, d] for i, d in cells), k


def check_against_mirror(eng, seqs, x, gammas=(0.5, 1.0, 4.0), mask_eng=None):
    """every structure and score equal to the mirror's over the same call's P (min_prob 0: every kept cell) and unpaired; with
    mask_eng (eng itself, or an engine with eng's batch resident when eng streams it) also well formed on its kept cells"""
    out = {}
    for gamma in gammas:
        structs, scores, prs = eng.mea_structures(x, gamma, 0.0)
        assert len(structs) == len(seqs) == len(scores) == len(prs)
        for k, seq in enumerate(seqs):
            L, W = len(seq), min(len(seq), eng.max_span)
            ii, jj, pp, unp = prs[k]
            P, kept = pair_matrix(L, W, ii, jj, pp)
            s, sc = mea_fold(P, kept, unp, gamma)
            assert structs[k] == s, (gamma, k)
            assert scores[k] == sc, (gamma, k, scores[k], sc)
            if mask_eng is not None:
                check_structure(mask_eng, k, L, structs[k])
        out[gamma] = structs, scores, prs
    return out


def check_scan(eng, x, seqs, refs):
    """scan records against the oracle's scan: start and inner in log space and exist_prob; where the oracle has a parse with the
    motif (exist_prob > 0) also end in log space and Ys, Ye, rss and psihat exact (where it has none, every start and inner
    posterior is -inf, the argmax is a tie and the oracle's end posteriors are 0 / 0); the batch's expected counts E[N] against
    the sum of the oracle's per sequence"""
    recs, en = eng.scan(x)
    assert len(recs) == len(seqs)
    np.testing.assert_allclose(en, np.sum([ref["scan"]["EN"] for ref in refs], axis=0), rtol=1e-8, atol=1e-10, err_msg="E[N] of the scan")
    for k, (r, ref) in enumerate(zip(recs, refs)):
        a = ref["scan"]
        assert_log_close(r["start"], a["start"], rtol=1e-8, atol=1e-6, what="start %d" % k)
        assert_log_close(r["inner"], a["inner"], rtol=1e-8, atol=1e-6, what="inner %d" % k)
        assert r["exist_prob"] == pytest.approx(a["exist_prob"], rel=1e-8), k
        if a["exist_prob"] == 0.0:
            continue
        assert_log_close(r["end"], a["end"], rtol=1e-8, atol=1e-6, what="end %d" % k)
        assert (r["Ys"], r["Ye"]) == (a["Ys"], a["Ye"]), (k, len(seqs[k]))
        assert r["rss"] == a["rss"], k
        assert list(r["psihat"]) == list(a["psihat"]), k
    return recs


def check_pair_path(eng, seqs, quals, x, make_oracle, gammas=GAMMAS, scan=False, refs=None, mask_eng=None, no_rss=False):
    """The whole check of one loaded batch: pair list, P and unpaired against the oracle (a sequence without a parse: P = 0,
    unpaired = 1); MEA structures and scores bit for bit against the mirror at every gamma; at OPT_GAMMAS the score equals the
    optimum over the oracle's P at rel 1e-9 and so does the expected accuracy of the structure; a sequence without a parse folds
    to all '.' with a score of exactly L.  scan: also the scan records against the oracle.  mask_eng: an engine with the same batch resident, for
    the kept cells when eng streams its batch.  no_rss: a model without secondary structure (--no-rss), under which no cell is
    kept and every sequence is checked as one without a parse (the oracle's plane P is no pair posterior there).  Returns
    (refs, pair_posteriors, mea by gamma)."""
    mask_eng = mask_eng or eng
    if refs is None:
        refs = oracle_refs(make_oracle, seqs, quals)
    Ps = [None if no_rss else r["P"] for r in refs]
    res = eng.pair_posteriors(x, 0.0)
    check_pair_lists(mask_eng, seqs, res, Ps)
    mea = check_against_mirror(eng, seqs, x, gammas, mask_eng)
    for gamma in gammas:
        structs, scores, _ = mea[gamma]
        for k, (seq, P) in enumerate(zip(seqs, Ps)):
            L = len(seq)
            if P is None:
                assert structs[k] == "." * L and scores[k] == float(L), (gamma, k, structs[k], scores[k])
                continue
            if gamma not in OPT_GAMMAS:
                continue
            kept = mask_eng.pairs(k)[0].astype(bool)
            Pk = P[:, :kept.shape[1]]
            q = unpaired_of(Pk, L)
            _, opt = mea_fold(Pk, kept, q, gamma)
            assert scores[k] == pytest.approx(opt, rel=1e-9), (gamma, k)
            assert expected_accuracy(structs[k], Pk, q, gamma) == pytest.approx(opt, rel=1e-9), (gamma, k)
    if scan:
        check_scan(eng, x, seqs, refs)
    return refs, res, mea
