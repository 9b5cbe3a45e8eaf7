"""Shared checks of the accessibility.  Two references built from the oracle alone -- enumerated_access
(every structure over the kept cells, weighted by the oracle's own fixed-structure partition function, added to each of its all-dot
windows) and table_access (the four path sums of access_rules.h in numpy over the oracle's inside / outside tables, with the
emission weights restated from the reference's rules as node_check.table_profile restates them) -- and the test-only CPU driver of
the product rule (tests/access_emul.cpp)."""
import ctypes as C
import os
import subprocess

import numpy as np

from oracle import pyoracle as po
from tests import ctx_check as cc
from tests import node_check as nc
from tests.emul import build as _emul_build

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "access_emul.cpp")
LIB = os.path.join(HERE, "libelemdp_access_emul.so")
TERMS = ("L", "O", "2", "M")
_lib = None

access_oracle = cc.ctx_oracle
access_oracle_from_model = cc.ctx_oracle_from_model


def nan_tail(L, U):
    """(L, U) mask of the windows that run off the end: p + w > L"""
    return np.add.outer(np.arange(L), np.arange(1, U + 1)) > L


def all_ones(L, U):
    """a sequence without any parse, a model without secondary structure"""
    a = np.ones((L, U))
    a[nan_tail(L, U)] = np.nan
    return a


# ---- enumeration ---------------------------------------------------------------------------------------------------------------------

def enumerated_access(o, seq, qual, U):
    """(L, U) accessibility by brute force, or None for a sequence without a parse"""
    L = len(seq)
    Zo = o.derivation_logz(seq, qual, None, None)
    if not np.isfinite(Zo):
        return None
    _, kept, _, _ = o.bpp(seq)
    W = kept.shape[1] - 1
    dbs = cc.structures(kept, L, W)
    assert len(set(dbs)) == len(dbs)
    assert len(dbs) <= cc.MAX_STRUCTURES, len(dbs)
    acc = np.zeros((L, U))
    total = 0.0
    for db in dbs:
        w = np.exp(o.derivation_logz(seq, qual, db, None) - Zo)
        if w == 0.0:
            continue
        total += w
        run = 0                                   # dots from p on
        for p in range(L - 1, -1, -1):
            run = run + 1 if db[p] == "." else 0
            acc[p, :min(run, U)] += w
    assert abs(total - 1.0) <= 1e-12, total
    acc[nan_tail(L, U)] = np.nan
    return acc


# ---- the four path sums over the oracle's tables ------------------------------------------------------------------------------------

def table_access(o, seq, qual, x, U, tau=0.1):
    """((L, U) accessibility, {term: (L, U) array by the window's start}) from the oracle's inside / outside tables of the first
    (full-terminal) pass, or None without a parse.  The oracle's dense tables are log 0 wherever a cell is not parsable in a plane,
    which stands for the guards of rules 3a and 5a; its out(2) is whole, so there is no pair-table part."""
    o.set_params(x)
    x = np.asarray(x, dtype=np.float64)
    seq = np.asarray(seq)
    L = len(seq)
    tail = nan_tail(L, U)
    t = o.train_seq(seq, qual, tables=True)
    Zo = t["Zo"]
    if not np.isfinite(Zo):
        return None
    if o.flags & po.NO_RSS:
        return all_ones(L, U), {k: np.zeros((L, U)) for k in TERMS}
    ins, outs, io_, oo = t["inside"], t["outside"], t["inside_o"], t["outside_o"]
    W = t["W"]
    hmm = o.hmm()
    names, tid, sizes = hmm["node"], hmm["theta_id"], hmm["theta_sizes"]
    states = [tuple(s) for s in hmm["state"]]
    S = len(states)
    sid = {s: k for k, s in enumerate(states)}
    lam = np.array([x[-2] if l == r else x[-1] for l, r in states])
    ne = bool(o.flags & po.NO_ENE)
    kept = o.bpp(seq)[1]
    if not np.isfinite(t["Zari"]):
        oo = cc.no_motif_outside_chain(o, seq, x, t, hmm, sid, kept, lam, ne)
    off = np.concatenate([[0], np.cumsum(sizes)])
    theta = [np.array(x[off[r]:off[r + 1]]) for r in range(len(sizes))]
    if o.flags & po.THETA_SOFTMAX:
        theta = [v - np.logaddexp.reduce(v) for v in theta]
    if o.flags & po.NO_PRF:
        theta = [np.zeros_like(v) for v in theta]
    ws = nc.position_weights(qual)
    ltau = np.log(tau)
    M_, T2_, L_ = 2, 5, 6
    NEG = -np.inf
    allpos = np.arange(L)

    def single(node):
        b = seq.astype(np.int64)
        w = np.where(b > 0, theta[tid[node]][np.maximum(b, 1) - 1], 0.0) if tid[node] >= 0 else np.zeros(L)
        return w + (ws[allpos] if names[node] in ".()" else 0.0)

    # the weight of every position for a right emission par -> ch (rules 3a, 8) and a left emission par -> ch (rule 5a)
    right = [(s, s1, single(states[s][1]) + (ltau if states[s][1] == states[s1][1] and names[states[s][1]] == "." else 0.0))
             for s in range(S) for s1 in hmm["right"][s]]
    left = [(s, sl, single(states[sl][0]) + (ltau if states[sl][0] == states[s][0] and names[states[sl][0]] == "." else 0.0))
            for s in range(S) for sl in hmm["left"][s]]

    def step(V, trans, pos, ok):
        """V[r, :] one emission further, row r at position pos[r]; rows with ok False die"""
        out = np.full_like(V, NEG)
        p = np.clip(pos, 0, L - 1)
        for s, c, w in trans:
            out[:, s] = np.logaddexp(out[:, s], V[:, c] + w[p])
        out[~ok] = NEG
        return out

    def post(V, O):
        with np.errstate(invalid="ignore", over="ignore"):
            return np.nan_to_num(np.exp(V + O - Zo), nan=0.0).sum(axis=1)

    terms = {k: np.zeros((L, U)) for k in TERMS}
    with np.errstate(invalid="ignore", over="ignore"):
        # T_L: u(i, d) along the column of the right end
        loops = np.array(hmm["loop_state"], dtype=int)
        u = np.nan_to_num(np.exp(ins[:, :, L_, loops] + outs[:, :, L_, loops] - Zo), nan=0.0).sum(axis=2)   # [i, d]
        for a in range(L):
            for w in range(1, U + 1):
                b = a + w
                if b > L:
                    break
                terms["L"][a, w - 1] = sum(u[b - d, d] for d in range(w, min(W, b) + 1))
        # T_O: every start a at once
        V = io_[:L, :].copy()
        for w in range(1, U + 1):
            pos = allpos + w - 1
            ok = pos < L
            V = step(V, right, pos, ok)
            terms["O"][:, w - 1] = np.where(ok, post(V, oo[np.clip(allpos + w, 0, L), :]), 0.0)
        # T_2: per span d0 of the start cell (k, d0), k = a - d0, every a at once
        for d0 in range(1, W):
            k = allpos - d0
            live = k >= 0
            kk = np.clip(k, 0, L)
            V = np.where(live[:, None], ins[kk, d0, T2_, :], NEG)
            for w in range(1, U + 1):
                if d0 + w > W:
                    break
                pos = allpos + w - 1
                ok = live & (pos < L)
                V = step(V, right, pos, ok)
                terms["2"][:, w - 1] += np.where(ok, post(V, outs[kk, d0 + w, T2_, :]), 0.0)
        # T_M: per span d0 of the start cell (b, d0), every end b at once; the window starts at b - w
        ends = np.arange(L + 1)
        for d0 in range(1, W):
            live = ends + d0 <= L
            V = np.where(live[:, None], ins[ends, d0, M_, :], NEG)
            for w in range(1, U + 1):
                if d0 + w > W:
                    break
                pos = ends - w
                ok = live & (pos >= 0)
                V = step(V, left, pos, ok)
                v = np.where(ok, post(V, outs[np.clip(pos, 0, L), d0 + w, M_, :]), 0.0)
                a = pos[ok]
                terms["M"][a, w - 1] += v[ok]
    acc = np.clip(terms["L"] + terms["O"] + terms["2"] + terms["M"], 0.0, 1.0)
    assert not np.isnan(acc).any()
    acc[tail] = np.nan
    return acc, terms


# ---- the CPU driver of the product rule ---------------------------------------------------------------------------------------------

def driver():
    global _lib
    if _lib is None:
        srcs = [SRC] + _emul_build.SRCS[1:]
        deps = [SRC] + _emul_build.DEPS + [os.path.join(_emul_build.CSRC, f) for f in ("access_rules.h", "node_rules.h", "ctx_rules.h", "pair_rules.h")]
        if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in deps):
            subprocess.check_call(["g++", "-std=c++14", "-O2", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-o", LIB] + srcs)
        L = C.CDLL(LIB)
        dp, u8 = C.POINTER(C.c_double), C.POINTER(C.c_uint8)
        L.emu_create.restype = C.c_void_p
        L.emu_create.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int]
        L.emu_destroy.argtypes = [C.c_void_p]
        L.emu_last_error.restype = C.c_char_p
        L.emu_set_fast.argtypes = [C.c_void_p, C.c_int]
        L.emu_access_seq.argtypes = [C.c_void_p, dp, u8, C.c_int, u8, C.c_int, C.c_int, dp, dp]
        _lib = L
    return _lib


class AccessDriver:
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

    def access(self, x, seq, qual, U, form=0):
        """((L, U) accessibility, {term: (L, U) array by the window's start}, the form that wrote them): form LIN hands a
        sequence on to LOG where Z leaves the double range or the sequence has no parse, as the engine does"""
        x = np.ascontiguousarray(x, dtype=np.float64)
        seq = np.ascontiguousarray(seq, dtype=np.uint8)
        qual = np.ascontiguousarray(qual, dtype=np.uint8)
        L = len(seq)
        acc = np.full(max(U * L, 1), -1.0)
        terms = np.full(max(4 * U * L, 1), -1.0)
        dp, u8 = C.POINTER(C.c_double), C.POINTER(C.c_uint8)
        rc = driver().emu_access_seq(self.h, x.ctypes.data_as(dp), seq.ctypes.data_as(u8), L, qual.ctypes.data_as(u8), form, U,
                                     acc.ctypes.data_as(dp), terms.ctypes.data_as(dp))
        if rc < 0:
            raise RuntimeError(driver().emu_last_error().decode())
        terms = terms[:4 * U * L].reshape(L, 4, U)
        return acc[:U * L].reshape(L, U), {k: terms[:, n, :] for n, k in enumerate(TERMS)}, rc


def assert_access(got, ref, what="", rtol=1e-8, atol=1e-10):
    """NaN exactly on the windows that run off the end; the project's `unpaired` tolerances elsewhere"""
    L, U = ref.shape
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    tail = nan_tail(L, U)
    assert np.array_equal(np.isnan(got), tail), what
    assert np.array_equal(np.isnan(ref), tail), what
    np.testing.assert_allclose(got[~tail], ref[~tail], rtol=rtol, atol=atol, err_msg=str(what))
    assert got[~tail].min(initial=0.0) >= 0.0 and got[~tail].max(initial=0.0) <= 1.0, what
