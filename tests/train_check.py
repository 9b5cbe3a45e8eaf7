"""Shared checks of the train path: one train evaluation of a loaded batch against the oracle, sequence
by sequence -- the seq_stats row (Zo, Zari, Znasi, f, skipped) and the count columns ENo, ENx, EHo, EHx that
elemdp_train_seq_counts reads back -- and as a batch (fn, gr, sum_eff, n_skipped, the count segments of train_partial).

Why the rows: under schedule 1 a sequence with the motif has gr = ENo - ENx = pn (B - A) with pn = Z(nasi) / Z of the order 1e-3,
so an error in the A sweep reaches the batch gradient a thousand times smaller and passes its rtol 1e-7 / atol 1e-7; ENo and ENx
each carry it in full (test_train_shapes_cpu.py: test_checker_sees_what_the_batch_gradient_hides).

The oracle work runs over the sequences of a batch in a thread pool (the oracle's C calls release the GIL), one oracle handle per
worker thread, as in tests/pair_check.py."""
import threading
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from tests.pair_check import n_workers
from tests.util import assert_log_close

COUNTS = ("ENo", "ENx", "EHo", "EHx")
# per-sequence counts: the project's tolerance for these quantities on the GPU (test_tables_of_single_sequences)
ROW_RTOL, ROW_ATOL = 1e-8, 1e-10
GR_TOL = dict(rtol=1e-7, atol=1e-7)          # the project's tolerance of the batch gradient

WORST = dict(err=0.0, where="")              # worst |gpu - oracle| / (atol / rtol + |oracle|) of a count any check has seen


class TrainRefs:
    """seq: Oracle.train_seq per sequence (without the chain tables); batch: Oracle.train_eval of the whole batch"""

    def __init__(self, seq, batch):
        self.seq, self.batch = seq, batch

    def unskipped(self, quals, first=0, count=None):
        """(with motif, without motif): the sequences of the window the oracle does not skip, by label"""
        count = len(self.seq) - first if count is None else count
        ks = [k for k in range(first, first + count) if not self.seq[k]["skipped"]]
        return sum(has_motif(quals[k]) for k in ks), sum(not has_motif(quals[k]) for k in ks)


def has_motif(qual):
    return int(qual[-1]) == 0


def label(qual):
    return "with motif" if has_motif(qual) else "without motif"


def relabelled(seqs, quals):
    """every sequence once with the motif (final quality 0) and once without (final quality 5): a fault tied to a length shows
    unattenuated in one of the two"""
    s2, q2 = [], []
    for s, q in zip(seqs, quals):
        for last in (0, 5):
            qq = q.copy()
            qq[-1] = last
            s2.append(s)
            q2.append(qq)
    return s2, q2


def oracle_train_refs(make_oracle, seqs, quals):
    """make_oracle() returns a fresh oracle handle with the parameters set, one per worker thread"""
    local = threading.local()

    def one(k):
        if not hasattr(local, "o"):
            local.o = make_oracle()
        r = local.o.train_seq(seqs[k], quals[k])
        del r["inside_o"], r["outside_o"]
        return r

    order = sorted(range(len(seqs)), key=lambda k: -len(seqs[k]))     # (longest first: the pool drains evenly)
    def whole():          # (beside the pool, on half the threads: the longest sequence bounds both)
        o = make_oracle()
        return o.train_eval(o.get_params(), seqs, quals, n_threads=max(1, n_workers() // 2)) if len(seqs) else None

    with ThreadPoolExecutor(max_workers=max(1, n_workers() // 2) + 1) as ex:
        batch = ex.submit(whole)
        done = dict(zip(order, ex.map(one, order)))
        batch = batch.result()
    return TrainRefs([done[k] for k in range(len(seqs))], batch)


def count_error(got, ref, rtol=ROW_RTOL, atol=ROW_ATOL):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        err = np.abs(got - ref) / (atol / rtol + np.abs(ref))
    return np.where(np.isfinite(got), err, np.inf)            # (a NaN or inf count is an error of any size)


def compare_counts(got, ref, where, rtol=ROW_RTOL, atol=ROW_ATOL, track=True):
    """got, ref: dicts of ENo, ENx, EHo, EHx of one sequence (or of a sum); raises naming the first column beyond the tolerance"""
    for key in COUNTS:
        err = count_error(got[key], ref[key], rtol, atol)
        if err.size == 0:
            continue
        j = int(np.argmax(err))
        if track and np.isfinite(err[j]) and err[j] > WORST["err"]:
            WORST.update(err=float(err[j]), where="%s %s[%d]" % (where, key, j))
        assert err[j] <= rtol, "%s: %s[%d] = %.17g, oracle %.17g (error %.3e of rtol %.1e / atol %.1e)" % (
            where, key, j, np.asarray(got[key])[j], np.asarray(ref[key])[j], err[j], rtol, atol)


def where_of(k, seqs, quals):
    return "sequence %d (L %d, %s)" % (k, len(seqs[k]), label(quals[k]))


def check_rows(stats, counts, refs, seqs, quals, first=0, count=None):
    """stats: seq_stats(); counts: seq_counts() or None; the rows first .. first + count against the oracle"""
    count = len(seqs) - first if count is None else count
    for k in range(first, first + count):
        a, st, w = refs.seq[k], stats[k], where_of(k, seqs, quals)
        for c, name in enumerate(("Zo", "Zari", "Znasi")):
            assert_log_close(st[c], a[name], rtol=1e-9, atol=1e-9, what="%s: %s = %.17g, oracle %.17g" % (w, name, st[c], a[name]))
        assert (st[4] != 0) == bool(a["skipped"]), "%s: skipped = %g, oracle %d" % (w, st[4], a["skipped"])
        if not a["skipped"]:
            assert st[3] == pytest.approx(a["f"], rel=1e-9), "%s: f = %.17g, oracle %.17g" % (w, st[3], a["f"])
        if counts is None:
            continue
        got = {key: counts[key][k] for key in COUNTS}
        if a["skipped"]:          # (k_reduce sums every row: a skipped sequence contributes nothing only because these stay 0)
            for key in COUNTS:
                nz = np.flatnonzero(got[key] != 0.0)
                assert nz.size == 0, "%s, skipped by the oracle: %s[%d] = %.17g, not exactly 0" % (w, key, nz[0], got[key][nz[0]])
        else:
            compare_counts(got, a, w)


def summed(refs, first, count):
    ks = [k for k in range(first, first + count) if not refs.seq[k]["skipped"]]
    tot = {key: np.sum([refs.seq[k][key] for k in ks], axis=0) if ks else np.zeros_like(refs.seq[first][key]) for key in COUNTS}
    return ks, tot


def partial_counts(part, nt):
    return dict(ENo=part[4:4 + nt], ENx=part[4 + nt:4 + 2 * nt], EHo=part[4 + 2 * nt:6 + 2 * nt], EHx=part[6 + 2 * nt:8 + 2 * nt])


def check_batch_sums(res, part, refs, seqs, quals, gr_ref, first, count, what=""):
    """res = (fn, gr, sum_eff, n_skipped) of train_eval, part = train_partial: against the sums over the oracle's sequences of the
    window, gr against the oracle's train_eval, and the four count segments of the partial vector one by one (a sum of n counts,
    each within rtol / atol of the oracle's: rtol on the sum, n atol)"""
    fn, gr, eff, nsk = res
    ks, tot = summed(refs, first, count)
    f_o = float(np.sum([refs.seq[k]["f"] for k in ks])) if ks else 0.0
    eff_o = float(np.sum([refs.seq[k]["bpp_eff"] for k in ks])) if ks else 0.0
    assert fn == pytest.approx(f_o, rel=1e-9, abs=1e-9), "%sfn = %.17g, oracle %.17g" % (what, fn, f_o)
    assert eff == pytest.approx(eff_o, rel=1e-12), "%ssum_eff = %.17g, oracle %.17g" % (what, eff, eff_o)
    assert nsk == count - len(ks), "%sn_skipped = %d, oracle %d" % (what, nsk, count - len(ks))
    np.testing.assert_allclose(gr, gr_ref, err_msg="%sgr against the oracle's train_eval" % what, **GR_TOL)
    nt = len(refs.seq[first]["ENo"])
    compare_counts(partial_counts(part, nt), tot, "%ssum over %d sequences" % (what, len(ks)), ROW_RTOL, ROW_ATOL * max(1, len(ks)),
                   track=False)
    assert part[0] == pytest.approx(f_o, rel=1e-9, abs=1e-9) and int(round(part[3])) == count - len(ks), (what, part[:4])


def check_train_path(eng, seqs, quals, x, make_oracle, refs=None, rows=True, window=None):
    """The whole check of one loaded batch (see the module's docstring): one train_eval, its rows and sums against the oracle;
    train_finish(train_partial(x)) against train_eval(x) at the tolerances of test_fn_gr_against_reference_golden; a second
    evaluation on the same slots repeats the first (fn rel 1e-12, rows 1e-10: nothing is left behind in the tables, which the
    suite poisons before every evaluation).  rows False: a streamed batch, without seq_counts.  window = (first, count): the
    options eval_first / eval_count, and that window's rows and sums only.  refs: oracle_train_refs of the batch at x when the
    caller has them.  Returns (refs, train_eval's result, seq_stats, seq_counts or None)."""
    if refs is None:
        refs = oracle_train_refs(make_oracle, seqs, quals)
    first, count = window if window is not None else (0, len(seqs))
    if window is not None:
        eng.set_option("eval_first", first)
        eng.set_option("eval_count", count)
        gr_ref = make_oracle().train_eval(x, seqs[first:first + count], quals[first:first + count], n_threads=n_workers())[1]
    else:
        gr_ref = refs.batch[1]
    what = "" if window is None else "window (%d, %d): " % (first, count)
    sl = slice(first, first + count)

    def rows_now():
        st = eng.seq_stats()
        return st, ({k: v.copy() for k, v in eng.seq_counts().items()} if rows else None)

    res = eng.train_eval(x)
    stats, counts = rows_now()
    check_rows(stats, counts, refs, seqs, quals, first, count)
    part = eng.train_partial(x)
    check_batch_sums(res, part, refs, seqs, quals, gr_ref, first, count, what)
    # the partial / finish pair (same numbers up to the order of the atomics that accumulate the expected counts)
    fn2, gr2, eff2, nsk2 = eng.train_finish(part)
    assert fn2 == pytest.approx(res[0], rel=1e-13) and eff2 == res[2] and nsk2 == res[3], (what, fn2, res[0], eff2, res[2])
    np.testing.assert_allclose(gr2, res[1], rtol=1e-11, atol=1e-12, err_msg=what + "train_finish(train_partial) against train_eval")
    # the second evaluation (train_partial above was the second on these slots; its rows, and a third)
    st2, c2 = rows_now()
    res3 = eng.train_eval(x)
    st3, c3 = rows_now()
    for st_n, c_n, fn_n in ((st2, c2, part[0]), (st3, c3, res3[0])):
        assert fn_n == pytest.approx(res[0], rel=1e-12), (what, fn_n, res[0])
        np.testing.assert_allclose(st_n[sl], stats[sl], rtol=1e-10, atol=1e-10, err_msg=what + "seq_stats of a repeated evaluation")
        for key in COUNTS if rows else ():
            np.testing.assert_allclose(c_n[key][sl], counts[key][sl], rtol=1e-10, atol=1e-10,
                                       err_msg=what + key + " of a repeated evaluation")
    np.testing.assert_allclose(res3[1], res[1], rtol=1e-11, atol=1e-12, err_msg=what + "gr of a repeated evaluation")
    if window is not None:
        eng.set_option("eval_first", 0)
        eng.set_option("eval_count", 0)
    return refs, res, stats, counts
