"""Shared checks of the pair posteriors by motif node pair.  Three references built from the oracle alone:
A. enumerated_stems -- every structure of ctx_check.structures times every node row of node_check.alignments, each weighted by
   the oracle's own derivation_logz; every pair (i, j) of the structure adds the weight to the node pair (row[i], row[j]);
B. table_stems -- the definition of stem_rules.h in numpy over the oracle's inside / outside tables: the 1a, 1b block of
   node_check.table_profile routed to the pair of nodes, the emission weights restated here;
C. assert_counts_equal_en -- the counts summed by pair type against the EN of the oracle's own scan;
and the test-only CPU driver of the product rule (tests/stem_emul.cpp).  The references are dense: Q[i, j, ml, mr], j exclusive."""
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
SRC = os.path.join(HERE, "stem_emul.cpp")
LIB = os.path.join(HERE, "libelemdp_stem_emul.so")
PARTS_ALL, PART_1A, PART_1B = 3, 1, 2
PAR = jc.PAR
CASES, case_id, tiny_inputs, stem_params = jc.CASES, jc.case_id, jc.tiny_inputs, jc.joint_params
stem_oracle, stem_oracle_from_model = jc.joint_oracle, jc.joint_oracle_from_model
assert_stem = jc.assert_joint                  # the project's rtol 1e-8, atol 1e-10, entry by entry
_lib = None
_refs = {}


def tiny_reference(case):
    """(x, seq, qual, oracle, enumerated Q) of an enumerated case, computed once per process"""
    if case not in _refs:
        pattern, _, flags, min_bpp = case
        x, s, q = tiny_inputs(case)
        o = stem_oracle(pattern, 50, 30, min_bpp=min_bpp, flags=flags)
        o.set_params(x)
        _refs[case] = (x, s, q, o, enumerated_stems(o, s, q))
    return _refs[case]


def db_pairs(db):
    stack, out = [], []
    for p, c in enumerate(db):
        if c == "(":
            stack.append(p)
        elif c == ")":
            out.append((stack.pop(), p))
    return out


# ---- A: enumeration ------------------------------------------------------------------------------------------------------------------

def enumerated_stems(o, seq, qual):
    """(L, L + 1, M, M) Q by brute force (the loop of joint_check.enumerated_joint), or None for a sequence without a parse"""
    L = len(seq)
    names = o.hmm()["node"]
    M = len(names)
    Zo = o.derivation_logz(seq, qual, None, None)
    if not np.isfinite(Zo):
        return None
    _, kept, _, _ = o.bpp(seq)
    W = kept.shape[1] - 1
    dbs = [db for db in cc.structures(kept, L, W) if np.isfinite(o.derivation_logz(seq, qual, db, None))]
    rows = [h for h in nc.alignments(L, names) if np.isfinite(o.derivation_logz(seq, qual, None, h))]
    assert len(dbs) <= cc.MAX_STRUCTURES and len(rows) <= nc.MAX_ROWS
    pairs = [db_pairs(db) for db in dbs]
    chars = np.array([list(db) for db in dbs]).reshape(len(dbs), L)
    is_open = np.array([c == "(" for c in names])
    is_close = np.array([c == ")" for c in names])
    Q = np.zeros((L, L + 1, M, M))
    total = 0.0
    for h in rows:
        fits = np.all((chars == "(") | ~is_open[h], axis=1) & np.all((chars == ")") | ~is_close[h], axis=1)
        for k in np.nonzero(fits)[0]:
            w = np.exp(o.derivation_logz(seq, qual, dbs[k], h) - Zo)
            if w == 0.0:
                continue
            total += w
            for i, j in pairs[k]:
                Q[i, j + 1, h[i], h[j]] += w
    assert abs(total - 1.0) <= 1e-12, total
    return Q


def pattern_pairs(names):
    """the (left node, right node) of every bracket pair of the pattern"""
    return sorted((l, r) for r, l in nc.bracket_partner(names).items())


# ---- B: the definition over the oracle's tables -----------------------------------------------------------------------------------------

def table_stems(o, seq, qual, x, tau=0.1, parts=PARTS_ALL):
    """(L, L + 1, M, M) Q from the oracle's inside / outside tables of the first (full-terminal) pass, or None without a parse
    (under NO_RSS: all zeros).  parts: the terms that take part (PART_* bits), for the test that shows a dropped term is seen."""
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
    M = len(names)
    Q = np.zeros((L, L + 1, M, M))
    if o.flags & po.NO_RSS:
        return Q
    states = [tuple(s) for s in hmm["state"]]
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
    tP, tE = 0, 1
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

    with np.errstate(invalid="ignore", over="ignore"):
        for d in range(2, W + 1):
            i = np.arange(0, L - d + 1)
            ik = i[kept[i, d] > 0]
            if not len(ik):
                continue
            est = np.array([0.0 if ne else o.loop_energy(seq, int(a), int(a) + d - 1, int(a) + 1, int(a) + d - 2) for a in ik])
            stack_ok = (kept[ik + 1, d - 2] > 0) & np.isfinite(est)
            est = np.where(stack_ok, est, 0.0)
            for s, (l, r) in enumerate(states):
                for sp in hmm["pair"][s]:
                    a = ins[ik + 1, d - 2, tE, sp] if parts & PART_1A else np.full(len(ik), NEG)
                    b = np.where(stack_ok, ins[ik + 1, d - 2, tP, sp] + lam[s] * est, NEG) if parts & PART_1B else np.full(len(ik), NEG)
                    v = outs[ik, d, tP, s] + w_pair(s, sp, ik, ik + d - 1) + np.logaddexp(a, b)
                    Q[ik, ik + d, states[sp][0], r] += np.nan_to_num(np.exp(v - Zo), nan=0.0)
    return np.clip(Q, 0.0, 1.0)


# ---- between the dense references and the product's slots ---------------------------------------------------------------------------------

def by_slot(Qd, slots):
    """(L, L + 1, K) of a dense reference on the product's slots; a slot the reference reaches must be among them"""
    slots = np.asarray(slots).reshape(-1, 2)
    on = np.zeros(Qd.shape[2:], dtype=bool)
    on[slots[:, 0], slots[:, 1]] = True
    assert not Qd[:, :, ~on].any(), "mass on a node pair that is no slot of the product"
    return Qd[:, :, slots[:, 0], slots[:, 1]]


def counts_of(Q, seq):
    """(K, 5, 5) counts of a Q[i, j, k]"""
    seq = np.asarray(seq)
    out = np.zeros((Q.shape[2], 5, 5))
    for i, j in zip(*np.nonzero(Q.any(axis=2))):
        out[:, seq[i], seq[j - 1]] += Q[i, j]
    return out


def dense_from_list(L, K, lst):
    """(L, L + 1, K) from the list (i, j, slot, q) of one sequence"""
    Q = np.zeros((L, L + 1, K))
    ii, jj, kk, q = lst
    Q[ii, jj, kk] = q
    return Q


def assert_counts_equal_en(o, seq, qual, counts, slots, what=""):
    """C: for every theta row of six pair types and every type, the counts summed over the slots whose right node owns the row
    and over the base pairs of the type = the oracle scan's EN there"""
    hmm = o.hmm()
    tid, sizes = hmm["theta_id"], hmm["theta_sizes"]
    slots = np.asarray(slots).reshape(-1, 2)
    sc = o.scan_seq(seq, qual)
    off = np.concatenate([[0], np.cumsum(sizes)])
    seen = 0
    for r, size in enumerate(sizes):
        if size != 6:
            continue
        mine = [k for k in range(len(slots)) if tid[slots[k, 1]] == r]
        for (bl, br), ty in nc.BP_TYPE.items():
            got = sum(counts[k, bl, br] for k in mine)
            np.testing.assert_allclose(got, sc["EN"][off[r] + ty - 1], rtol=1e-8, atol=1e-10, err_msg="row %d type %d %s" % (r, ty, what))
            seen += 1
    return seen


# ---- the CPU driver of the product rule ---------------------------------------------------------------------------------------------

def driver():
    global _lib
    if _lib is None:
        srcs = [SRC] + _emul_build.SRCS[1:]
        deps = [SRC] + _emul_build.DEPS + [os.path.join(_emul_build.CSRC, f) for f in ("stem_rules.h", "node_rules.h", "ctx_rules.h", "pair_rules.h")]
        if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in deps):
            subprocess.check_call(["g++", "-std=c++14", "-O2", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-o", LIB] + srcs)
        L = C.CDLL(LIB)
        dp, u8, i32 = C.POINTER(C.c_double), C.POINTER(C.c_uint8), C.POINTER(C.c_int32)
        L.emu_create.restype = C.c_void_p
        L.emu_create.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int]
        L.emu_destroy.argtypes = [C.c_void_p]
        L.emu_last_error.restype = C.c_char_p
        L.emu_set_fast.argtypes = [C.c_void_p, C.c_int]
        L.emu_stem_slots.argtypes = [C.c_void_p, i32, i32, C.c_int]
        L.emu_stem_span.argtypes = [C.c_void_p, u8, C.c_int, u8]
        L.emu_stem_seq.argtypes = [C.c_void_p, dp, u8, C.c_int, u8, C.c_int, C.c_int, dp, dp]
        _lib = L
    return _lib


class StemDriver:
    LIN, LOG = 0, 1

    def __init__(self, pattern, par="~T2004~", max_span=50, max_iloop=30, min_bpp=1e-4, tau=0.1, flags=0):
        if par in ("~T2004~", "~A2007~"):
            par = po.energy_param_text(par)
        self.h = driver().emu_create(pattern.encode(), par.encode(), max_span, max_iloop, min_bpp, tau, flags)
        if not self.h:
            raise RuntimeError(driver().emu_last_error().decode())
        i32 = C.POINTER(C.c_int32)
        K = driver().emu_stem_slots(self.h, None, None, 0)
        left, right = (np.zeros(max(K, 1), dtype=np.int32) for _ in range(2))
        driver().emu_stem_slots(self.h, left.ctypes.data_as(i32), right.ctypes.data_as(i32), K)
        self.slots = np.stack([left[:K], right[:K]], axis=1)

    def __del__(self):
        try:
            driver().emu_destroy(self.h)
        except Exception:
            pass

    def set_fast(self, on):
        driver().emu_set_fast(self.h, int(bool(on)))

    def stems(self, x, seq, qual, form=0, parts=PARTS_ALL):
        """((L, L + 1, K) Q, (K, 5, 5) counts, the form that wrote them): form LIN hands a sequence on to LOG where Z leaves the
        double range or the sequence has no parse, as the engine does"""
        x = np.ascontiguousarray(x, dtype=np.float64)
        seq = np.ascontiguousarray(seq, dtype=np.uint8)
        qual = np.ascontiguousarray(qual, dtype=np.uint8)
        L, K = len(seq), len(self.slots)
        dp, u8 = C.POINTER(C.c_double), C.POINTER(C.c_uint8)
        W = driver().emu_stem_span(self.h, seq.ctypes.data_as(u8), L, qual.ctypes.data_as(u8))
        if W < 0:
            raise RuntimeError(driver().emu_last_error().decode())
        raw = np.full(max((L + 1) * (W + 1) * K, 1), np.nan)
        counts = np.full(max(25 * K, 1), np.nan)
        rc = driver().emu_stem_seq(self.h, x.ctypes.data_as(dp), seq.ctypes.data_as(u8), L, qual.ctypes.data_as(u8), form, parts,
                                   raw.ctypes.data_as(dp), counts.ctypes.data_as(dp))
        if rc < 0:
            raise RuntimeError(driver().emu_last_error().decode())
        raw = raw[:(L + 1) * (W + 1) * K].reshape(K, W + 1, L + 1)
        Q = np.zeros((L, L + 1, K))
        for d in range(W + 1):
            i = np.arange(0, min(L - d + 1, L))
            Q[i, i + d] = raw[:, d, i].T
        assert not np.isnan(Q).any()
        return Q, counts[:25 * K].reshape(K, 5, 5), rc
