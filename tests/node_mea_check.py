"""Shared checks of the maximum expected accuracy motif alignments and site lists.  Two references, neither
of which uses product code:
A. brute_sites -- every row of node_check.alignments scored, the maximum under the exclusions slot by slot, with the margin to
   the second best score;
B. dp_sites -- a plain numpy chain recursion over the positions, for lengths the enumeration cannot afford, which also accepts a
   list of given exclusions;
a checker that holds a result of any length against B without depending on how ties were broken; and the test-only CPU driver of
the product rule (tests/node_mea_emul.cpp)."""
import ctypes as C
import os
import subprocess

import numpy as np

from tests import node_check as nc

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
SRC = os.path.join(HERE, "node_mea_emul.cpp")
LIB = os.path.join(HERE, "libelemdp_node_mea_emul.so")
RULES = os.path.join(REPO, "rnaelem_amd", "csrc", "node_mea_rules.h")
PROFILE_ATOL = 1e-10        # the absolute tolerance assert_profile (ctx_check) applies to a profile entry
_lib = None


def gains(M, gamma):
    g = np.full(M, float(gamma))
    g[0] = g[M - 1] = 1.0
    return g


def row_score(prof, row, gamma):
    prof = np.asarray(prof)
    row = np.asarray(row, dtype=np.int64)
    return float((gains(prof.shape[1], gamma)[row] * prof[np.arange(len(row)), row]).sum())


def valid_row(row, names):
    """is the row that of some alignment?  (the chain form of the definition)"""
    row = [int(v) for v in row]
    M = len(names)
    if not row or any(v < 0 or v >= M for v in row):
        return False

    def stars_between(a, b):
        return all(names[k] == "*" for k in range(a + 1, b))

    if not (row[0] == 0 or (0 < row[0] < M - 1 and stars_between(0, row[0]))):
        return False
    for a, b in zip(row, row[1:]):
        if b == a:
            continue
        if b < a or (a == 0 and b == M - 1) or not stars_between(a, b):
            return False
    last = row[-1]
    return last == 0 or last == M - 1 or stars_between(last, M - 1)


def site_of(row, M):
    """(start, end) of the positions that carry inner nodes, or None"""
    inner = np.nonzero((np.asarray(row) > 0) & (np.asarray(row) < M - 1))[0]
    if len(inner) == 0:
        return None
    assert inner[-1] - inner[0] + 1 == len(inner), row
    return int(inner[0]), int(inner[-1]) + 1


def barred_mask(L, sites):
    bar = np.zeros(L, dtype=bool)
    for a, b in sites:
        bar[a:b] = True
    return bar


# ---- A: enumeration -----------------------------------------------------------------------------------------------------------------

def brute_sites(prof, names, gamma, K):
    """[(row, (start, end), score, margin)] slot by slot until the all-z row wins (that slot is the last entry, with site None)
    or K slots are filled; margin = best score - second best score among the rows allowed in that slot"""
    prof = np.asarray(prof)
    L, M = prof.shape
    rows = np.array(list(nc.alignments(L, names)), dtype=np.int64)
    assert len(rows) <= nc.MAX_ROWS, len(rows)
    g = gains(M, gamma)
    scores = (g[rows] * prof[np.arange(L)[None, :], rows]).sum(axis=1)
    inner = (rows > 0) & (rows < M - 1)
    out, sites = [], []
    for _ in range(K):
        ok = ~(inner & barred_mask(L, sites)[None, :]).any(axis=1)
        cand = np.nonzero(ok)[0]
        order = cand[np.argsort(-scores[cand], kind="stable")]
        best = order[0]
        margin = float(scores[best] - scores[order[1]]) if len(order) > 1 else np.inf
        site = site_of(rows[best], M)
        out.append((rows[best].astype(np.uint8), site, float(scores[best]), margin))
        if site is None:
            break
        sites.append(site)
    return out


# ---- B: chain recursion --------------------------------------------------------------------------------------------------------------

def chain_lists(names):
    """(preds, first, last) from the definition"""
    M = len(names)

    def stars_between(a, b):
        return all(names[k] == "*" for k in range(a + 1, b))

    preds = [[a for a in range(m + 1) if a == m or (stars_between(a, m) and not (a == 0 and m == M - 1))] for m in range(M)]
    first = [m == 0 or (0 < m < M - 1 and stars_between(0, m)) for m in range(M)]
    last = [m == 0 or m == M - 1 or stars_between(m, M - 1) for m in range(M)]
    return preds, first, last


def dp_best(prof, names, gamma, excluded=()):
    """(score, row) of the best valid row that puts no inner node on a position of the excluded sites"""
    prof = np.asarray(prof)
    L, M = prof.shape
    preds, first, last = chain_lists(names)
    g = gains(M, gamma)
    bar = barred_mask(L, excluded)
    mask = np.zeros((M, M), dtype=bool)         # mask[m, a]: a is a predecessor of m
    for m in range(M):
        mask[m, preds[m]] = True
    inner = (np.arange(M) > 0) & (np.arange(M) < M - 1)
    V = np.full((L, M), -np.inf)
    back = np.zeros((L, M), dtype=np.int64)
    if L:
        V[0] = np.where(np.array(first) & ~(inner & bar[0]), g * prof[0], -np.inf)
    for p in range(1, L):
        cand = np.where(mask, V[p - 1][None, :], -np.inf)
        back[p] = cand.argmax(axis=1)            # (the first of the greatest: the lowest predecessor)
        best = cand[np.arange(M), back[p]]
        V[p] = np.where(inner & bar[p], -np.inf, g * prof[p] + best)
    fin = max((m for m in range(M) if last[m]), key=lambda m: (V[L - 1, m], -m))
    row = np.zeros(L, dtype=np.uint8)
    m = fin
    for p in range(L - 1, -1, -1):
        row[p] = m
        m = back[p, m]
    return float(V[L - 1, fin]), row


def dp_sites(prof, names, gamma, K, excluded=()):
    """[(row, site, score)] slot by slot as brute_sites, the sites of `excluded` barred from the start"""
    M = len(names)
    out, sites = [], list(excluded)
    for _ in range(K):
        score, row = dp_best(prof, names, gamma, sites)
        site = site_of(row, M)
        out.append((row, site, score))
        if site is None:
            break
        sites.append(site)
    return out


# ---- the tie-robust checker ---------------------------------------------------------------------------------------------------------

def check_result(res, ref_prof, names, gamma, K, own_prof=None, what=""):
    """res: dict(rows (n_sites, L), start, end, score, confidence) of one sequence and, as `slots`, optionally the raw K slots
    (rows (K, L), start, end, score, confidence of every slot).  Every slot against B's maximum under the exclusions the result
    itself reported; the reported numbers recomputed from the row."""
    ref_prof = np.asarray(ref_prof)
    L, M = ref_prof.shape
    ns = len(res["start"])
    assert res["rows"].shape == (ns, L) and ns <= K, (what, res["rows"].shape, ns)
    tol = L * max(gamma, 1.0) * PROFILE_ATOL
    sites = []
    for k in range(ns):
        row = res["rows"][k]
        assert valid_row(row, names), (what, k, row)
        site = site_of(row, M)
        assert site is not None and site == (int(res["start"][k]), int(res["end"][k])), (what, k, site)
        bar = barred_mask(L, sites)
        assert not (bar & (row > 0) & (row < M - 1)).any(), (what, k, "overlaps an earlier site")
        best, _ = dp_best(ref_prof, names, gamma, sites)
        assert abs(row_score(ref_prof, row, gamma) - best) <= tol, (what, k, row_score(ref_prof, row, gamma), best)
        prof = ref_prof if own_prof is None else own_prof
        if own_prof is not None:
            own_best, _ = dp_best(own_prof, names, gamma, sites)
            assert abs(row_score(own_prof, row, gamma) - own_best) <= 1e-12 * max(abs(own_best), 1.0), (what, k)
        ptol = tol if own_prof is None else 1e-12 * max(L * max(gamma, 1.0), 1.0)
        assert abs(res["score"][k] - row_score(prof, row, gamma)) <= ptol, (what, k, res["score"][k])
        conf = prof[np.arange(site[0], site[1]), row[site[0]:site[1]]].mean()
        assert abs(res["confidence"][k] - conf) <= (PROFILE_ATOL if own_prof is None else 1e-12), (what, k, res["confidence"][k], conf)
        sites.append(site)
    if ns < K:      # the list ended because all z won the next slot
        best, row = dp_best(ref_prof, names, gamma, sites)
        assert abs(row_score(ref_prof, np.zeros(L, dtype=np.int64), gamma) - best) <= tol, (what, "slot %d is not all z" % ns, best, row)
    if "slots" in res:
        s = res["slots"]
        assert s["rows"].shape == (K, L)
        assert np.array_equal(s["rows"][:ns], res["rows"]) and not s["rows"][ns:].any(), what
        assert np.all(s["start"][ns:] == -1) and np.all(s["end"][ns:] == -1), what
        assert np.all(np.isnan(s["score"][ns:])) and np.all(np.isnan(s["confidence"][ns:])), what
    return sites


# ---- the CPU driver of the product rule ---------------------------------------------------------------------------------------------

def driver():
    global _lib
    if _lib is None:
        deps = [SRC, RULES, os.path.join(os.path.dirname(RULES), "dp_rules.h")]
        if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in deps):
            subprocess.check_call(["g++", "-std=c++14", "-O2", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-o", LIB, SRC])
        L = C.CDLL(LIB)
        dp, u8, i32 = C.POINTER(C.c_double), C.POINTER(C.c_uint8), C.POINTER(C.c_int32)
        L.emu_node_mea_lists.argtypes = [C.c_char_p, C.c_int, i32]
        L.emu_node_mea_seq.argtypes = [C.c_char_p, C.c_int, C.c_int, dp, C.c_double, C.c_int, u8, i32, i32, dp, dp]
        _lib = L
    return _lib


def driver_lists(names):
    """(lo, first, last) of node_mea_lists_build"""
    M = len(names)
    out = np.zeros(3 * M, dtype=np.int32)
    driver().emu_node_mea_lists(names.encode(), M, out.ctypes.data_as(C.POINTER(C.c_int32)))
    return out[:M], out[M:2 * M], out[2 * M:]


def rows_of_lists(lo, first, last, L):
    """every row the chain lists generate, as a set of tuples"""
    M = len(lo)
    rows = [(m,) for m in range(M) if first[m]]
    for _ in range(L - 1):
        rows = [r + (m,) for r in rows for m in range(M) if lo[m] <= r[-1] <= m]
    return {r for r in rows if last[r[-1]]}


def driver_sites(prof, names, gamma, K):
    """the result of one sequence in the form Engine.mea_alignments gives, with the raw slots as `slots`"""
    prof = np.ascontiguousarray(prof, dtype=np.float64)
    L, M = prof.shape
    flat = np.full(max(K * L, 1), 255, dtype=np.uint8)
    s0, s1 = np.zeros(K, dtype=np.int32), np.zeros(K, dtype=np.int32)
    sc, cf = np.zeros(K), np.zeros(K)
    dp, u8, i32 = C.POINTER(C.c_double), C.POINTER(C.c_uint8), C.POINTER(C.c_int32)
    ns = driver().emu_node_mea_seq(names.encode(), M, L, prof.ctypes.data_as(dp), float(gamma), K, flat.ctypes.data_as(u8),
                                   s0.ctypes.data_as(i32), s1.ctypes.data_as(i32), sc.ctypes.data_as(dp), cf.ctypes.data_as(dp))
    if ns < 0:
        raise ValueError("refused")
    rows = flat[:K * L].reshape(K, L)
    return dict(rows=rows[:ns].copy(), start=s0[:ns].copy(), end=s1[:ns].copy(), score=sc[:ns].copy(), confidence=cf[:ns].copy(),
                slots=dict(rows=rows, start=s0, end=s1, score=sc, confidence=cf))


def assert_equals_brute(res, brute, what=""):
    """rows, sites and scores of a result equal reference A's (whose last entry is the all-z slot where the list ended)"""
    want = [b for b in brute if b[1] is not None]
    assert len(res["start"]) == len(want), (what, len(res["start"]), len(want))
    for k, (row, site, score, _) in enumerate(want):
        assert np.array_equal(res["rows"][k], row), (what, k, res["rows"][k], row)
        assert (int(res["start"][k]), int(res["end"][k])) == site, (what, k)
        assert abs(res["score"][k] - score) <= 1e-12 * max(abs(score), 1.0), (what, k, res["score"][k], score)
