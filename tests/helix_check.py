"""Shared checks of the helix posteriors.  Three references, none of them the code under test:
A. enumerated_helices -- every structure of ctx_check.structures weighted by the oracle's own derivation_logz; every pair of the
   structure adds the weight to (i, j, k) for every k its nesting reaches.  It knows nothing of rules;
B. table_helices -- the definition of helix_rules.h in numpy over the oracle's inside / outside tables, the weights restated here
   as stem_check.table_stems restates them;
C. HelixDriver -- the test-only CPU driver of the product rule (tests/helix_emul.cpp), for lengths where B is slow.
The references are dense: H[i, j, k - 1], j exclusive, 0 where the helix (i, j, k) does not fit the kept cells."""
import ctypes as C
import os
import subprocess

import numpy as np

from oracle import pyoracle as po
from tests import ctx_check as cc
from tests import joint_check as jc
from tests import node_check as nc
from tests.emul import build as _emul_build

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "helix_emul.cpp")
LIB = os.path.join(HERE, "libelemdp_helix_emul.so")
PAR = jc.PAR
case_id, tiny_inputs, helix_params = jc.case_id, jc.tiny_inputs, jc.joint_params
# the enumerated cases of joint_check and one longer one: at 13 bases no structure of .(.*). nests three pairs; at 16 bases (462
# structures, far below ctx_check.MAX_STRUCTURES) its best helix of three pairs has 0.136
CASES = jc.CASES + [(".(.*).", 16, 0, 1e-4)]
helix_oracle, helix_oracle_from_model = jc.joint_oracle, jc.joint_oracle_from_model
assert_helix = jc.assert_joint                  # the project's rtol 1e-8, atol 1e-10, entry by entry
KMAX = 8                                        # lengths of the dense references (no enumerated case nests deeper than 4)
_lib = None
_refs = {}


def tiny_reference(case):
    """(x, seq, qual, oracle, enumerated H) of an enumerated case, computed once per process"""
    if case not in _refs:
        pattern, _, flags, min_bpp = case
        x, s, q = tiny_inputs(case)
        o = helix_oracle(pattern, 50, 30, min_bpp=min_bpp, flags=flags)
        o.set_params(x)
        _refs[case] = (x, s, q, o, enumerated_helices(o, s, q))
    return _refs[case]


def mates(db):
    mate, stack = [-1] * len(db), []
    for p, c in enumerate(db):
        if c == "(":
            stack.append(p)
        elif c == ")":
            mate[p] = stack.pop()
            mate[mate[p]] = p
    return mate


# ---- A: enumeration ------------------------------------------------------------------------------------------------------------------

def enumerated_helices(o, seq, qual, kmax=KMAX):
    """(L, L + 1, kmax) H by brute force (the loop of access_check.enumerated_access), or None for a sequence without a parse"""
    L = len(seq)
    Zo = o.derivation_logz(seq, qual, None, None)
    if not np.isfinite(Zo):
        return None
    _, kept, _, _ = o.bpp(seq)
    W = kept.shape[1] - 1
    dbs = cc.structures(kept, L, W)
    assert len(set(dbs)) == len(dbs)
    assert len(dbs) <= cc.MAX_STRUCTURES, len(dbs)
    H = np.zeros((L, L + 1, kmax))
    total = 0.0
    for db in dbs:
        w = np.exp(o.derivation_logz(seq, qual, db, None) - Zo)
        if w == 0.0:
            continue
        total += w
        mate = mates(db)
        for a, b in enumerate(mate):
            if b < a:
                continue
            k = 0
            while a + k < b - k and mate[a + k] == b - k:
                assert k < kmax
                H[a, b + 1, k] += w
                k += 1
    assert abs(total - 1.0) <= 1e-12, total
    return H


# ---- B: the definition over the oracle's tables -----------------------------------------------------------------------------------------

def table_helices(o, seq, qual, x, tau=0.1, kmax=KMAX):
    """(L, L + 1, kmax) H from the oracle's inside / outside tables of the first (full-terminal) pass, or None without a parse
    (under NO_RSS: all zeros): per kept cell the vector out(P, i, d, .) stepped inward along the stacking rule."""
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
    H = np.zeros((L, L + 1, kmax))
    if o.flags & po.NO_RSS:
        return H
    states = [tuple(s) for s in hmm["state"]]
    S = len(states)
    lam = np.array([x[-2] if l == r else x[-1] for l, r in states])
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
    tP = 0
    ty_of = np.zeros((5, 5), dtype=np.int64)
    for (bi, bj), ty in nc.BP_TYPE.items():
        ty_of[bi, bj] = ty
    NEG = -np.inf

    def single(node, pos):
        b = seq[pos].astype(np.int64)
        w = np.where(b > 0, theta[tid[node]][np.maximum(b, 1) - 1], 0.0) if tid[node] >= 0 else np.zeros(len(pos))
        return w + (ws[pos] if names[node] in ".()" else 0.0)

    def w_pair(par, ch, pi, pj):
        # a ')' node owns a row of six pair types and emits both bases jointly; any other right node emits two single bases
        r, l = states[par][1], states[ch][0]
        if names[r] == ")":
            ty = ty_of[seq[pi].astype(np.int64), seq[pj].astype(np.int64)]
            w = np.where(ty > 0, theta[tid[r]][np.maximum(ty, 1) - 1], 0.0)
            w = w + (ws[pi] if names[l] in ".()" else 0.0) + ws[pj]
        else:
            w = single(l, pi) + single(r, pj)
        return w + (ltau if r == states[ch][1] and names[r] == ")" else 0.0)

    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for d in range(2, W + 1):
            i = np.arange(0, L - d + 1)
            i0 = i[kept[i, d] > 0]
            if not len(i0):
                continue
            V = outs[i0, d, tP, :].astype(np.float64).copy()          # (n, S), the vector of every chain of this diagonal
            on = np.ones(len(i0), dtype=bool)
            for k in range(1, kmax + 1):
                ik, dk = i0 + k - 1, d - 2 * (k - 1)
                dot = np.logaddexp.reduce(np.where(on[:, None], V + ins[np.where(on, ik, 0), dk, tP, :], NEG), axis=1)
                H[i0[on], i0[on] + d, k - 1] = np.nan_to_num(np.exp(dot[on] - Zo), nan=0.0)
                if k == kmax or dk - 2 < 2:
                    break
                on = on & (kept[np.minimum(ik + 1, L), dk - 2] > 0)
                if not on.any():
                    break
                est = np.array([0.0 if ne else o.loop_energy(seq, int(a), int(a) + dk - 1, int(a) + 1, int(a) + dk - 2) if ok else NEG
                                for a, ok in zip(ik, on)])
                on = on & np.isfinite(est)
                est = np.where(on, est, 0.0)
                ia = np.where(on, ik, 0)
                V1 = np.full_like(V, NEG)
                for s in range(S):
                    for sp in hmm["pair"][s]:
                        V1[:, sp] = np.logaddexp(V1[:, sp], V[:, s] + w_pair(s, sp, ia, ia + dk - 1) + lam[s] * est)
                V = np.where(on[:, None], V1, NEG)
    return np.clip(H, 0.0, 1.0)


# ---- between the dense references, the lists and the properties ---------------------------------------------------------------------------

def dense_from_list(L, kmax, lst):
    """(L, L + 1, kmax) from the list (i, j, len, p) of one sequence"""
    H = np.zeros((L, L + 1, kmax))
    ii, jj, kk, p = lst
    H[ii, jj, kk - 1] = p
    return H


def assert_list_order(L, lst, min_len, max_len, what=""):
    """(i, j, len) strictly increasing, lengths in range and, per cell, min_len .. its last length without a gap; p in [0, 1]"""
    ii, jj, kk, p = lst
    key = (ii.astype(np.int64) * (L + 1) + jj) * 64 + kk
    assert np.all(np.diff(key) > 0), what
    if not len(kk):
        return
    assert kk.min() >= min_len and kk.max() <= max_len, what
    first = np.concatenate([[True], (ii[1:] != ii[:-1]) | (jj[1:] != jj[:-1])])
    assert np.all(kk[first] == min_len) and np.all(kk[1:][~first[1:]] == kk[:-1][~first[1:]] + 1), what
    assert p.min() >= 0.0 and p.max() <= 1.0, what


def assert_properties(H, tol, what=""):
    """non-increasing in k; H(i, d, k) <= H(i + 1, d - 2, k - 1)"""
    assert np.all(H[:, :, 1:] <= H[:, :, :-1] + tol), what
    inner = np.zeros_like(H[:, :, :-1])
    inner[:-1, 1:] = H[1:, :-1, :-1]                                     # (the cell (i + 1, j - 1) at length k - 1)
    assert np.all(H[:, :, 1:] <= inner + tol), what


# ---- the CPU driver of the product rule ---------------------------------------------------------------------------------------------

def driver():
    global _lib
    if _lib is None:
        srcs = [SRC] + _emul_build.SRCS[1:]
        deps = [SRC] + _emul_build.DEPS + [os.path.join(_emul_build.CSRC, f) for f in
                                           ("helix_rules.h", "access_rules.h", "node_rules.h", "ctx_rules.h", "pair_rules.h")]
        if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in deps):
            subprocess.check_call(["g++", "-std=c++14", "-O2", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-o", LIB] + srcs)
        L = C.CDLL(LIB)
        dp, u8, i32 = C.POINTER(C.c_double), C.POINTER(C.c_uint8), C.POINTER(C.c_int32)
        L.emu_create.restype = C.c_void_p
        L.emu_create.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int]
        L.emu_destroy.argtypes = [C.c_void_p]
        L.emu_last_error.restype = C.c_char_p
        L.emu_set_fast.argtypes = [C.c_void_p, C.c_int]
        L.emu_helix_span.argtypes = [C.c_void_p, u8, C.c_int, u8]
        L.emu_helix_seq.argtypes = [C.c_void_p, dp, u8, C.c_int, u8, C.c_int, C.c_int, C.c_double, dp, C.c_int, i32, i32, i32, dp]
        _lib = L
    return _lib


class HelixDriver:
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

    def helices(self, x, seq, qual, form=0, kmax=KMAX, min_prob=0.0, stems=()):
        """((L, L + 1, kmax) H, the joint probabilities of the stems (i, j, len), the form that wrote them): form LIN hands a
        sequence on to LOG where Z leaves the double range or the sequence has no parse, as the engine does"""
        x = np.ascontiguousarray(x, dtype=np.float64)
        seq = np.ascontiguousarray(seq, dtype=np.uint8)
        qual = np.ascontiguousarray(qual, dtype=np.uint8)
        L = len(seq)
        dp, u8, i32 = C.POINTER(C.c_double), C.POINTER(C.c_uint8), C.POINTER(C.c_int32)
        W = driver().emu_helix_span(self.h, seq.ctypes.data_as(u8), L, qual.ctypes.data_as(u8))
        if W < 0:
            raise RuntimeError(driver().emu_last_error().decode())
        raw = np.full(max(kmax * (L + 1) * (W + 1), 1), np.nan)
        ns = len(stems)
        si = np.array([s[0] for s in stems] + [0], dtype=np.int32)
        sd = np.array([s[1] - s[0] for s in stems] + [0], dtype=np.int32)
        sl = np.array([s[2] for s in stems] + [0], dtype=np.int32)
        sp = np.full(ns + 1, np.nan)
        rc = driver().emu_helix_seq(self.h, x.ctypes.data_as(dp), seq.ctypes.data_as(u8), L, qual.ctypes.data_as(u8), form, kmax,
                                    float(min_prob), raw.ctypes.data_as(dp), ns, si.ctypes.data_as(i32), sd.ctypes.data_as(i32),
                                    sl.ctypes.data_as(i32), sp.ctypes.data_as(dp))
        if rc < 0:
            raise RuntimeError(driver().emu_last_error().decode())
        raw = raw[:kmax * (W + 1) * (L + 1)].reshape(kmax, W + 1, L + 1)
        H = np.zeros((L, L + 1, kmax))
        for d in range(W + 1):
            i = np.arange(0, min(L - d + 1, L))
            H[i, i + d] = raw[:, d, i].T
        assert not np.isnan(H).any() and not np.isnan(sp[:ns]).any()
        return H, sp[:ns], rc
