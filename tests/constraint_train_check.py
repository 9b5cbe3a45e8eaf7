"""The train row of a constrained sequence by enumeration (Tests), from the oracle alone: Zo, Zari, Znasi, f,
skipped and the count vectors ENo, ENx, EHo, EHx that train_check.check_rows compares, for the strings of
constraint_check.enumerated_cases().

The constrained ensemble is the set of structures that satisfy the string.  An oracle made with DBG_FIX_RSS gives the train row of
ONE structure s (train_seq(fix_rss=s)): Z_s of the three terminal sets and the four count vectors, each a conditional expectation
in the ensemble of one terminal set.  The row of a set of structures is the Z-weighted mixture, X = sum_s exp(Z_s - Z) X_s with
Z = logaddexp_s Z_s, where Z is the partition function of the ensemble the vector belongs to (ensemble_keys):

    label                         ENo, EHo     ENx, EHx      f
    with motif (final quality 0)  Zo           Zari          Zo - Zari
    without motif                 Zo           Znasi         Zo - Znasi
    without motif, LIK_RATIO      Zari         Zo            Zari - Zo

One trap.  The oracle skips a structure that has no parse with the motif (Zari_s = -inf): it returns the structure's Zo_s and
Znasi_s but zeros for its counts, so a Zo- or Znasi-weighted sum over such a structure loses its share.  Vectors of the Zari
ensemble are never affected (a skipped structure has weight 0 there).  For the others there are two routes:

    direct       the mixture over the satisfying structures, where the oracle skips none of them with weight in that ensemble;
    complement   Z_c X_c = Z X_free - sum over the structures that do NOT satisfy the string, with X_free from the free oracle's
                 train_seq; valid where none of those is skipped with weight, and where every satisfying structure is a structure
                 of the free mask (the string brings no pair back that the filter dropped).  The route is refused where the
                 constrained ensemble's share Zo_c / Zo is below MIN_SHARE.  The error of the result is that of the terms over
                 the share of the vector's own ensemble (row["share_o"], row["share_x"]), which may be smaller than Zo_c / Zo:
                 with terms good to 1e-14 times counts of at most 10, a share of 5e-4 leaves 2e-10 / 10 of train_check.ROW_ATOL.

A vector that neither route serves is left out of the row (its key is missing, row["parts"] says which are there)."""
import threading
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from oracle import pyoracle as po
from tests import constraint_check as kc
from tests import ctx_check as cc
from tests import joint_check as jc
from tests import train_check as tc
from tests.pair_check import n_workers

MIN_SHARE = 1e-3
LABELS = (0, 5)          # the final quality: with the motif, without it
ZKEYS = ("Zo", "Zari", "Znasi")

_rows = {}               # (case, flags, final quality) -> {dot-bracket: row of the one structure}
_free = {}               # (case, flags, final quality) -> the free oracle's row
_refs = {}               # (case, flags, final quality, string) -> the constrained row


def labelled(qual, last):
    q = np.array(qual, dtype=np.uint8)
    q[-1] = last
    return q


def ensemble_keys(flags, with_motif):
    """(the Z of ENo and EHo, the Z of ENx and EHx, f as (plus, minus)): elem_oracle.cpp, train_seq_impl"""
    if with_motif:
        return "Zo", "Zari", ("Zo", "Zari")
    if flags & po.LIK_RATIO:
        return "Zari", "Zo", ("Zari", "Zo")
    return "Zo", "Znasi", ("Zo", "Znasi")


def case_oracle(case, flags, x):
    pattern, _, _, min_bpp = case
    o = jc.joint_oracle(pattern, 50, 30, min_bpp=min_bpp, flags=flags)
    o.set_params(x)
    return o


def structure_rows(case, flags, x, seq, qual, dbs):
    """{db: train_seq(fix_rss=db) of the DBG_FIX_RSS oracle, without the chain tables} for the label of qual; cached per process,
    the missing ones through a thread pool with one oracle handle per worker"""
    assert not flags & (po.THETA_SOFTMAX | po.NO_RSS)
    have = _rows.setdefault((case, flags, int(qual[-1])), {})
    todo = [db for db in dict.fromkeys(dbs) if db not in have]
    local = threading.local()

    def one(db):
        if not hasattr(local, "o"):
            local.o = case_oracle(case, flags | po.DBG_FIX_RSS, x)
        r = local.o.train_seq(seq, qual, fix_rss=db)
        del r["inside_o"], r["outside_o"]
        return r

    if todo:
        with ThreadPoolExecutor(max_workers=n_workers()) as ex:
            have.update(zip(todo, ex.map(one, todo)))
    return have


def free_row(case, flags, x, seq, qual):
    key = (case, flags, int(qual[-1]))
    if key not in _free:
        r = case_oracle(case, flags, x).train_seq(seq, qual)
        del r["inside_o"], r["outside_o"]
        _free[key] = r
    return _free[key]


def logsum(v):
    v = np.asarray(v, dtype=np.float64)
    return float(np.logaddexp.reduce(v)) if v.size and np.isfinite(v).any() else -np.inf


def mixed_z(rows):
    return {k: logsum([r[k] for r in rows]) for k in ZKEYS}


def weighted(rows, zkey, z, keys):
    """sum_s exp(Z_s - z) X_s for the vectors `keys` over rows of finite Z_s"""
    out = None
    for r in rows:
        if np.isfinite(r[zkey]):
            w = np.exp(r[zkey] - z)
            term = [w * r[k] for k in keys]
            out = term if out is None else [a + b for a, b in zip(out, term)]
    return out


def lost(rows, zkey):
    """the structures the oracle skipped although they carry weight in the ensemble zkey: their counts came back as zeros"""
    return [r for r in rows if r["skipped"] and np.isfinite(r[zkey])]


def mixture_row(flags, qual, sat, others, free, complement_ok=True, force=None):
    """The train row of the structures `sat` (rows of structure_rows).  others: the rows of the remaining structures of the free
    mask and free: the free oracle's row, for the complement route (complement_ok: every row of sat is a structure of the free
    mask).  force: "direct" or "complement", to take that route for every vector it is valid for (the Zari ensemble is always
    direct) and leave out the others.  Returns the row with parts = {"o": route, "x": route} (route None: the vectors are
    missing) and share = exp(Zo_c - Zo)."""
    with_motif = tc.has_motif(qual)
    zo_key, zx_key, (fp, fm) = ensemble_keys(flags, with_motif)
    nt = len(free["ENo"])
    Z = mixed_z(sat)
    row = dict(Z, bpp_eff=free["bpp_eff"], L=free["L"], W=free["W"], parts={}, share=float(np.exp(Z["Zo"] - free["Zo"])))
    row["skipped"] = int(not (np.isfinite(Z["Zo"]) and np.isfinite(Z["Zari"])))
    if row["skipped"]:
        row.update(f=0.0, ENo=np.zeros(nt), ENx=np.zeros(nt), EHo=np.zeros(2), EHx=np.zeros(2), parts=dict(o="skipped", x="skipped"))
        return row
    row["f"] = Z[fp] - Z[fm]
    for part, zkey, keys in (("o", zo_key, ("ENo", "EHo")), ("x", zx_key, ("ENx", "EHx"))):
        direct = zkey == "Zari" or not lost(sat, zkey)
        share = float(np.exp(Z[zkey] - free[zkey]))
        comp = zkey != "Zari" and complement_ok and not lost(others, zkey) and row["share"] >= MIN_SHARE
        if force is None or zkey == "Zari":
            route = "direct" if direct else "complement" if comp else None
        else:
            route = force if (direct if force == "direct" else comp) else None
        row["parts"][part] = route
        if route == "direct":
            vals = weighted(sat, zkey, Z[zkey], keys)
        elif route == "complement":
            rest = weighted(others, zkey, free[zkey], keys) or [0.0, 0.0]
            vals = [(free[k] - r) / share for k, r in zip(keys, rest)]
        else:
            continue
        row.update(zip(keys, vals))
        row["share_" + part] = share
    return row


def case_structures(case, flags, x, seq):
    """(every structure over the oracle's mask, the mask)"""
    _, kept, _, _ = case_oracle(case, flags, x).bpp(seq)
    kept = np.asarray(kept, dtype=np.uint8)
    L = len(seq)
    return cc.structures(kept, L, kept.shape[1] - 1), kept


def constrained_row(case, x, seq, qual, cons, e, last, flags=None, force=None):
    """The reference row of the string cons under the label `last` (LABELS); e: the string's reference of
    constraint_check.enumerated (its dbs are the satisfying structures of weight).  flags: the case's own unless given (the
    structure set does not depend on LIK_RATIO)."""
    flags = case[2] if flags is None else flags
    key = (case, flags, last, cons, force)
    if key in _refs:
        return _refs[key]
    q = labelled(qual, last)
    free = free_row(case, flags, x, seq, q)
    all_dbs, kept = case_structures(case, flags, x, seq)
    sat_dbs = e.get("dbs", [])
    L = len(seq)
    kept_c, _ = kc.apply(kept, seq, cons, L, kept.shape[1] - 1)
    inside = bool(np.all(kept_c <= kept)) and set(sat_dbs) <= set(all_dbs)
    rows = structure_rows(case, flags, x, seq, q, list(all_dbs) + list(sat_dbs))
    sat_set = set(sat_dbs)
    # (a satisfying structure of weight 0 is in neither list of e: it adds nothing to either side)
    others = [rows[db] for db in all_dbs if db not in sat_set and not kc.satisfies(db, cons)]
    row = mixture_row(flags, q, [rows[db] for db in sat_dbs], others, free, complement_ok=inside, force=force)
    _refs[key] = row
    return row


# seed0 of constraint_check.case_strings per case of joint_check.CASES, for the strings this module adds to those of
# constraint_check.enumerated_cases(): chosen, from the oracle alone, so that at most one drawn string in four is left without the
# Zo- and Znasi-weighted vectors (tests/test_constraint_train_cpu.py asserts it).  Under `((.*.))` and `.(.*).` most structures
# have no parse with the motif and are skipped by the fixed-structure oracle, so that only a string whose forced pairs leave no
# such structure (direct route), or drop all of them (complement route), gets these vectors.
SEEDS = (5300, 6500, 7250, 8450, 9000, 10000, 11000, 12000, 13100, 14550, 15050, 16000, 17000)
_cases = {}


def train_cases():
    """constraint_check.enumerated_cases() with, for the cases of joint_check.CASES, the strings drawn at SEEDS behind the case's
    own: [(case, x, seq, qual, [(string, reference of constraint_check.enumerated)], n_own)], n_own = how many of the strings are
    the case's own; cached per process"""
    if "all" not in _cases:
        assert len(SEEDS) == len(jc.CASES)
        out = []
        for n, (case, x, s, q, refs) in enumerate(kc.enumerated_cases()):
            refs = list(refs)
            n_own = len(refs)
            if n < len(jc.CASES):
                assert case == jc.CASES[n]
                o = case_oracle(case, case[2], x)
                for c in kc.case_strings(o, s, tries=50, seed0=SEEDS[n]):
                    if c not in [c0 for c0, _ in refs]:
                        refs.append((c, kc.enumerated(o, s, q, c)))
            out.append((case, x, s, q, refs, n_own))
        _cases["all"] = out
    return _cases["all"]


def batch_of(case, x, seq, qual, refs, flags=None, labels=LABELS):
    """(seqs, quals, strings, rows) twice for one enumerated case: the batch of the complete rows -- per label a free copy (the
    free oracle's row), then every string whose row has all four vectors -- and the batch of the rows that lack some"""
    flags = case[2] if flags is None else flags
    full, part = ([], [], [], []), ([], [], [], [])
    for last in labels:
        q = labelled(qual, last)
        for c, row in [(None, free_row(case, flags, x, seq, q))] + [
                (c, constrained_row(case, x, seq, qual, c, e, last, flags=flags)) for c, e in refs]:
            for lst, v in zip(full if complete(row) else part, (seq, q, c, row)):
                lst.append(v)
    return full, part


def complete(row):
    return all(k in row for k in tc.COUNTS)


def gr_of(rows, n_param):
    """the batch gradient of reference rows (theta not softmax): sum of ENo - ENx, then EHo - EHx, over the unskipped rows"""
    gr = np.zeros(n_param)
    for r in rows:
        if not r["skipped"]:
            gr[:-2] += r["ENo"] - r["ENx"]
            gr[-2:] += r["EHo"] - r["EHx"]
    return gr


def train_refs(rows, n_param, first=0, count=None):
    """train_check.TrainRefs of reference rows; batch = (fn, gr, sum_eff, n_skipped) of the window"""
    count = len(rows) - first if count is None else count
    win = [r for r in rows[first:first + count] if not r["skipped"]]
    batch = (float(sum(r["f"] for r in win)), gr_of(win, n_param), float(sum(r["bpp_eff"] for r in win)), count - len(win))
    return tc.TrainRefs(list(rows), batch)


def check_window(eng, x, refs, seqs, quals, first, count):
    """one eval_first / eval_count window of a loaded batch against its rows' sums (check_train_path's window takes its gradient
    from the free oracle's train_eval, which knows no constraint)"""
    eng.set_option("eval_first", first)
    eng.set_option("eval_count", count)
    try:
        res = eng.train_eval(x)
        stats = eng.seq_stats()
        counts = {k: v.copy() for k, v in eng.seq_counts().items()}
        tc.check_rows(stats, counts, refs, seqs, quals, first, count)
        part = eng.train_partial(x)
        win = train_refs(refs.seq, len(x), first, count)
        tc.check_batch_sums(res, part, refs, seqs, quals, win.batch[1], first, count, "window (%d, %d): " % (first, count))
    finally:
        eng.set_option("eval_first", 0)
        eng.set_option("eval_count", 0)
    return res


def check_partial_rows(stats, counts, rows, seqs, quals):
    """rows that lack some vectors: Zo, Zari, Znasi, f and skipped as train_check.check_rows has them, and the vectors that are
    there at its tolerances"""
    tc.check_rows(stats, None, tc.TrainRefs(rows, None), seqs, quals)
    n = 0
    for k, row in enumerate(rows):
        for key in tc.COUNTS:
            if key in row:
                err = tc.count_error(counts[key][k], row[key])
                j = int(np.argmax(err))
                assert err[j] <= tc.ROW_RTOL, "%s: %s[%d] = %.17g, reference %.17g" % (
                    tc.where_of(k, seqs, quals), key, j, counts[key][k][j], row[key][j])
                n += 1
    return n
