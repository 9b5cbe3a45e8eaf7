"""Shared checks of the loop posteriors.  Three references, none of them the code under test:
A. enumerated_loops -- every structure of ctx_check.structures weighted by the oracle's own derivation_logz and decomposed pair by
   pair as ctx_check.classify does, stacks split off from the one-inner-pair case.  It knows nothing of rules;
B. table_loops -- the definitions of loop_rules.h in numpy over the oracle's inside / outside tables, the weights restated here as
   stem_check.table_stems and ctx_check.table_profile restate them;
C. LoopDriver -- the test-only CPU driver of the product rule (tests/loop_emul.cpp), for lengths where B is slow.
A reference is (cols, two): cols[i, j, c] dense, j exclusive, columns H S B I M; two a dict {(i, j, k, l): T}."""
import ctypes as C
import os
import subprocess

import numpy as np

from oracle import pyoracle as po
from tests import ctx_check as cc
from tests import helix_check as hc
from tests import joint_check as jc
from tests import node_check as nc
from tests.emul import build as _emul_build

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "loop_emul.cpp")
LIB = os.path.join(HERE, "libelemdp_loop_emul.so")
PAR = jc.PAR
case_id, tiny_inputs, loop_params = jc.case_id, jc.tiny_inputs, jc.joint_params
CASES = hc.CASES + [("(.*)", 18, po.NO_ENE, 0.0)]
loop_oracle, loop_oracle_from_model = jc.joint_oracle, jc.joint_oracle_from_model
assert_loop = jc.assert_joint                   # the project's rtol 1e-8, atol 1e-10, entry by entry
H_, S_, B_, I_, M_ = range(5)
LETTERS = "HSBIM"
_lib = None
_refs = {}


def tiny_reference(case):
    """(x, seq, qual, oracle, (enumerated cols, enumerated two-loops)) of an enumerated case, computed once per process"""
    if case not in _refs:
        pattern, _, flags, min_bpp = case
        x, s, q = tiny_inputs(case)
        o = loop_oracle(pattern, 50, 30, min_bpp=min_bpp, flags=flags)
        o.set_params(x)
        _refs[case] = (x, s, q, o, enumerated_loops(o, s, q))
    return _refs[case]


def loops_of(db):
    """(type 1 .. 5 for H S B I M, i, j, k, l) of every pair of a dot-bracket, by increasing i: the pair of the bases i and j-1 and
    the loop it closes; (k, l) is the inner pair's cell for a bulge or an interior loop and (-1, -1) otherwise"""
    mate = hc.mates(db)
    out = []
    for a, b in enumerate(mate):
        if b < a:
            continue
        inner, p = [], a + 1
        while p < b:
            if mate[p] > p:
                inner.append((p, mate[p]))
                p = mate[p] + 1
            else:
                p += 1
        if not inner:
            out.append((1, a, b + 1, -1, -1))
        elif len(inner) > 1:
            out.append((5, a, b + 1, -1, -1))
        else:
            k, l = inner[0]
            if k == a + 1 and l == b - 1:
                out.append((2, a, b + 1, -1, -1))
            else:
                out.append((3 if (k == a + 1) != (l == b - 1) else 4, a, b + 1, k, l + 1))
    return out


# ---- A: enumeration ------------------------------------------------------------------------------------------------------------------

def enumerated_loops(o, seq, qual):
    """((L, L + 1, 5) cols, {(i, j, k, l): T}) by brute force, or None for a sequence without a parse"""
    L = len(seq)
    Zo = o.derivation_logz(seq, qual, None, None)
    if not np.isfinite(Zo):
        return None
    _, kept, _, _ = o.bpp(seq)
    W = kept.shape[1] - 1
    dbs = cc.structures(kept, L, W)
    assert len(set(dbs)) == len(dbs)
    assert len(dbs) <= cc.MAX_STRUCTURES, len(dbs)
    cols = np.zeros((L, L + 1, 5))
    two = {}
    total = 0.0
    for db in dbs:
        w = np.exp(o.derivation_logz(seq, qual, db, None) - Zo)
        if w == 0.0:
            continue
        total += w
        for t, i, j, k, l in loops_of(db):
            cols[i, j, t - 1] += w
            if t in (3, 4):
                two[(i, j, k, l)] = two.get((i, j, k, l), 0.0) + w
    assert abs(total - 1.0) <= 1e-12, total
    return cols, two


# ---- B: the definitions over the oracle's tables -----------------------------------------------------------------------------------------

def table_loops(o, seq, qual, x, tau=0.1):
    """((L, L + 1, 5) cols, {(i, j, k, l): T}, (L, L + 1) P) from the oracle's inside / outside tables of the first (full-terminal)
    pass, or None without a parse (under NO_RSS: all zeros)"""
    o.set_params(x)
    x = np.asarray(x, dtype=np.float64)
    seq = np.asarray(seq)
    L = len(seq)
    t = o.train_seq(seq, qual, tables=True)
    Zo = t["Zo"]
    if not np.isfinite(Zo):
        return None
    ins, outs = t["inside"], t["outside"]
    W = t["W"]
    hmm = o.hmm()
    names, tid, sizes = hmm["node"], hmm["theta_id"], hmm["theta_sizes"]
    cols = np.zeros((L, L + 1, 5))
    P = np.zeros((L, L + 1))
    two = {}
    if o.flags & po.NO_RSS:
        return cols, two, P
    states = [tuple(s) for s in hmm["state"]]
    S = len(states)
    lam = np.array([x[-2] if l == r else x[-1] for l, r in states])
    loops = np.array(hmm["loop_state"], dtype=int)
    qd = np.array(hmm["loop_loop"], dtype=int).reshape(-1, 4)
    ne = bool(o.flags & po.NO_ENE)
    kept = o.bpp(seq)[1]
    off = np.concatenate([[0], np.cumsum(sizes)])
    theta = [np.array(x[off[r]:off[r + 1]]) for r in range(len(sizes))]
    if o.flags & po.THETA_SOFTMAX:
        theta = [v - np.logaddexp.reduce(v) for v in theta]
    if o.flags & po.NO_PRF:
        theta = [np.zeros_like(v) for v in theta]
    ws = nc.position_weights(qual)
    ltau = np.log(tau)
    C_ = min(W - 2 - 5, o.max_iloop_)
    m_min = 4 if o.flags & po.DBG_NO_TURN else 10
    ml_close = 0.0 if ne else float(o.energy_table("mlclosing")[0] + o.energy_table("mlintern")[0])
    tP, tE, tM, tL = 0, 1, 2, 6

    def single(node, pos):
        b = int(seq[pos])
        w = theta[tid[node]][b - 1] if tid[node] >= 0 and b > 0 else 0.0
        return w + (ws[pos] if names[node] in ".()" else 0.0)

    def w_pair(par, ch, pi, pj):
        # a ')' node owns a row of six pair types and emits both bases jointly; any other right node emits two single bases
        r, l = states[par][1], states[ch][0]
        if names[r] == ")":
            ty = nc.BP_TYPE.get((int(seq[pi]), int(seq[pj])), 0)
            w = theta[tid[r]][ty - 1] if ty > 0 else 0.0
            w = w + (ws[pi] if names[l] in ".()" else 0.0) + ws[pj]
        else:
            w = single(l, pi) + single(r, pj)
        return w + (ltau if r == states[ch][1] and names[r] == ")" else 0.0)

    def post(v):
        with np.errstate(invalid="ignore", over="ignore"):
            return float(np.nan_to_num(np.exp(np.asarray(v, dtype=np.float64) - Zo), nan=0.0).sum())

    for i in range(L + 1):
        for d in range(2, W + 1):
            j = i + d
            if j > L:
                break
            if not kept[i, d]:
                continue
            P[i, j] = post(ins[i, d, tP, :] + outs[i, d, tP, :])
            ie, de, je = i + 1, d - 2, j - 1
            # S: rule 1b
            if de >= 2 and kept[ie, de]:
                est = 0.0 if ne else o.loop_energy(seq, i, j - 1, i + 1, j - 2)
                if np.isfinite(est):
                    cols[i, j, S_] = post([outs[i, d, tP, s] + w_pair(s, sp, i, j - 1) + lam[s] * est + ins[ie, de, tP, sp]
                                           for s in range(S) for sp in hmm["pair"][s]] or [-np.inf])
            # H: rule 6b
            tsc = 0.0 if ne else o.hairpin_energy(seq, i, j - 1)
            if np.isfinite(tsc):
                cols[i, j, H_] = post(outs[ie, de, tE, loops] + lam[loops] * tsc + ins[ie, de, tL, loops])
            # M: rule 6a
            if 0 < ie and je < L and de <= W and m_min <= de:
                tsc = ml_close if ne else o.sum_ext_m(seq, j - 1, i, False) + ml_close
                if np.isfinite(tsc):
                    cols[i, j, M_] = post(outs[ie, de, tE, :] + lam * tsc + ins[ie, de, tM, :])
            # the two-loops: rule 6c over the inside enumeration
            for l in range(je, ie, -1):
                for k in range(ie, l):
                    u1, u2 = k - ie, je - l
                    if (u1 == 0 and u2 == 0) or u1 + u2 > C_ or not kept[k, l - k]:
                        continue
                    tsc = 0.0 if ne else o.loop_energy(seq, i, je, k, l - 1)
                    if not np.isfinite(tsc):
                        continue
                    w = post(outs[ie, de, tE, qd[:, 0]] + lam[qd[:, 0]] * tsc + ins[k, l - k, tP, qd[:, 1]] + ins[ie, k - ie, tL, qd[:, 2]]
                             + ins[l, je - l, tL, qd[:, 3]])
                    two[(i, j, k, l)] = min(max(w, 0.0), 1.0)
                    cols[i, j, B_ if (u1 == 0) != (u2 == 0) else I_] += w
    return np.clip(cols, 0.0, 1.0), two, P


# ---- between the references, the lists and the identities ---------------------------------------------------------------------------------

def dense_from_closing(L, lst):
    """((L, L + 1, 5) cols, (L, L + 1) p) from the closing list (i, j, p, cols) of one sequence"""
    ii, jj, p, c = lst
    cols, P = np.zeros((L, L + 1, 5)), np.zeros((L, L + 1))
    cols[ii, jj] = c
    P[ii, jj] = p
    return cols, P


def two_dict(lst):
    ii, jj, kk, ll, t = lst
    d = {(int(a), int(b), int(c), int(e)): float(v) for a, b, c, e, v in zip(ii, jj, kk, ll, t)}
    assert len(d) == len(t)
    return d


def assert_two(got, ref, what="", floor=0.0):
    """two dicts keyed by (i, j, k, l): every entry of either side above the floor is in the other, within the tolerance"""
    keys = sorted(set(got) | set(ref))
    g = np.array([got.get(k, 0.0) for k in keys])
    r = np.array([ref.get(k, 0.0) for k in keys])
    if floor > 0.0:   # (an entry within rounding of the threshold may be on one side only)
        edge = (np.abs(np.maximum(g, r) - floor) <= 1e-8 * floor + 1e-10) & ((g == 0.0) | (r == 0.0))
        g, r = g[~edge], r[~edge]
    assert_loop(g, r, what=what)


def range_add(L, runs):
    """(L,) the sum over the runs (a, b, v) of v on [a, b)"""
    diff = np.zeros(L + 1)
    for a, b, v in runs:
        diff[a] += v
        diff[b] -= v
    return np.cumsum(diff)[:L]


def assert_identities(L, cols, P, two, h2, profile, tol, what=""):
    """the identities of the issue on one sequence: cols (L, L + 1, 5), P and h2 (L, L + 1), two the full dict (min_prob 0),
    profile (L, 7) the context profile of the same tables"""
    assert np.abs(cols.sum(axis=2) - P).max() <= tol, (what, np.abs(cols.sum(axis=2) - P).max())
    assert np.abs(cols[:, :, S_] - h2).max() <= tol, what
    ii, jj = np.nonzero(cols[:, :, H_])
    assert np.abs(range_add(L, [(i + 1, j - 1, cols[i, j, H_]) for i, j in zip(ii, jj)]) - profile[:, 3]).max() <= tol, what
    bul, itr, per = [], [], {}
    for (i, j, k, l), v in two.items():
        per[(i, j)] = per.get((i, j), 0.0) + v
        if (k == i + 1) != (l == j - 1):
            bul.append((i + 1, k, v) if k > i + 1 else (l, j - 1, v))
        else:
            itr += [(i + 1, k, v), (l, j - 1, v)]
    assert np.abs(range_add(L, bul) - profile[:, 4]).max() <= tol, what
    assert np.abs(range_add(L, itr) - profile[:, 5]).max() <= tol, (what, np.abs(range_add(L, itr) - profile[:, 5]).max())
    got = np.zeros((L, L + 1))
    for (i, j), v in per.items():
        got[i, j] = v
    assert np.abs(got - cols[:, :, B_] - cols[:, :, I_]).max() <= tol, what


# ---- the CPU driver of the product rule ---------------------------------------------------------------------------------------------

def driver():
    global _lib
    if _lib is None:
        srcs = [SRC] + _emul_build.SRCS[1:]
        deps = [SRC] + _emul_build.DEPS + [os.path.join(_emul_build.CSRC, f) for f in
                                           ("loop_rules.h", "helix_rules.h", "access_rules.h", "node_rules.h", "ctx_rules.h", "pair_rules.h")]
        if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in deps):
            subprocess.check_call(["g++", "-std=c++14", "-O2", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-o", LIB] + srcs)
        L = C.CDLL(LIB)
        dp, u8, i32, i64 = C.POINTER(C.c_double), C.POINTER(C.c_uint8), C.POINTER(C.c_int32), C.POINTER(C.c_int64)
        L.emu_create.restype = C.c_void_p
        L.emu_create.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int]
        L.emu_destroy.argtypes = [C.c_void_p]
        L.emu_last_error.restype = C.c_char_p
        L.emu_set_fast.argtypes = [C.c_void_p, C.c_int]
        L.emu_loop_span.argtypes = [C.c_void_p, u8, C.c_int, u8]
        L.emu_loop_seq.argtypes = [C.c_void_p, dp, u8, C.c_int, u8, C.c_int, C.c_double, dp, dp, dp, dp, C.c_int64, i64, i32, i32, i32,
                                   i32, dp, C.c_int, i32, i32, i32, i32, i32, dp]
        _lib = L
    return _lib


class LoopDriver:
    LIN, LOG = 0, 1

    def __init__(self, pattern, par="~T2004~", max_span=50, max_iloop=30, min_bpp=1e-4, tau=0.1, flags=0):
        if par in ("~T2004~", "~A2007~"):
            par = po.energy_param_text(par)
        self.h = driver().emu_create(pattern.encode(), par.encode(), max_span, max_iloop, min_bpp, tau, flags)
        if not self.h:
            raise RuntimeError(driver().emu_last_error().decode())

    def __del__(self):
        try:
            driver().emu_destroy(self.h)
        except Exception:
            pass

    def set_fast(self, on):
        driver().emu_set_fast(self.h, int(bool(on)))

    def loops(self, x, seq, qual, form=0, min_prob=0.0, loops=()):
        """dict(cols (L, L + 1, 5), P, h2 (L, L + 1), two {(i, j, k, l): T} in list order, profile (L, 7), loops: the probabilities
        of the given loops (type, i, j, k, l), form: the form that wrote them).  form LIN hands a sequence on to LOG where Z leaves
        the double range or the sequence has no parse, as the engine does.  With min_prob > 0 the driver walks the cells the
        product walks: cols is 0 where P is below the pick bound."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        seq = np.ascontiguousarray(seq, dtype=np.uint8)
        qual = np.ascontiguousarray(qual, dtype=np.uint8)
        L = len(seq)
        dp, u8, i32 = C.POINTER(C.c_double), C.POINTER(C.c_uint8), C.POINTER(C.c_int32)
        W = driver().emu_loop_span(self.h, seq.ctypes.data_as(u8), L, qual.ctypes.data_as(u8))
        if W < 0:
            raise RuntimeError(driver().emu_last_error().decode())
        nc_ = (L + 1) * (W + 1)
        raw = np.full(5 * nc_, np.nan)
        rp, rh = np.full(nc_, np.nan), np.full(nc_, np.nan)
        prof = np.full(max(7 * L, 1), np.nan)
        ns = len(loops)
        cols5 = [np.array([s[c] for s in loops] + [0], dtype=np.int32) for c in range(5)]
        cols5[2] = cols5[2] - cols5[1]      # (j -> d)
        sp = np.full(ns + 1, np.nan)
        cap = 1 << 12
        while True:
            n_two = C.c_int64()
            t4 = [np.zeros(cap, dtype=np.int32) for _ in range(4)]
            tp = np.zeros(cap)
            rc = driver().emu_loop_seq(self.h, x.ctypes.data_as(dp), seq.ctypes.data_as(u8), L, qual.ctypes.data_as(u8), form,
                                       float(min_prob), raw.ctypes.data_as(dp), rp.ctypes.data_as(dp), rh.ctypes.data_as(dp),
                                       prof.ctypes.data_as(dp), cap, C.byref(n_two), *[a.ctypes.data_as(i32) for a in t4],
                                       tp.ctypes.data_as(dp), ns, *[a.ctypes.data_as(i32) for a in cols5], sp.ctypes.data_as(dp))
            if rc < 0:
                raise RuntimeError(driver().emu_last_error().decode())
            if n_two.value <= cap:
                break
            cap = int(n_two.value)
        m = n_two.value
        raw = raw.reshape(5, W + 1, L + 1)
        cols, P, h2 = np.zeros((L, L + 1, 5)), np.zeros((L, L + 1)), np.zeros((L, L + 1))
        for d in range(W + 1):
            i = np.arange(0, min(L - d + 1, L))
            cols[i, i + d] = raw[:, d, i].T
            P[i, i + d] = rp.reshape(W + 1, L + 1)[d, i]
            h2[i, i + d] = rh.reshape(W + 1, L + 1)[d, i]
        assert not np.isnan(cols).any() and not np.isnan(P).any() and not np.isnan(sp[:ns]).any()
        two = {(int(a), int(b), int(c), int(e)): float(v) for a, b, c, e, v in zip(*(a[:m] for a in t4), tp[:m])}
        assert len(two) == m
        return dict(cols=cols, P=P, h2=h2, two=two, profile=prof[:7 * L].reshape(L, 7), loops=sp[:ns], form=rc, W=W)
