"""Shared checks of the posterior motif-node profile.  Three references, none of which uses product code:
A. enumerated_profile -- every node row z* n1^r1 .. nk^rk o* weighted by the oracle's own derivation_logz;
B. oracle_identities -- what Oracle.scan_seq says about the same table: the inner posterior and the expected emission counts;
C. table_profile -- the definitions of node_rules.h in numpy over the oracle's inside / outside tables, with the emission
   weights restated here from the reference's rules (theta row of the emitting node, position weight, tau on a self-loop);
and the test-only CPU driver of the product rule (tests/node_emul.cpp)."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np

from oracle import pyoracle as po
from tests import ctx_check as cc
from tests.emul import build as _emul_build

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "node_emul.cpp")
LIB = os.path.join(HERE, "libelemdp_node_emul.so")
MAX_ROWS = 50000
_lib = None

node_oracle = cc.ctx_oracle
node_oracle_from_model = cc.ctx_oracle_from_model
assert_profile = cc.assert_profile


# ---- A: enumeration ------------------------------------------------------------------------------------------------------------------

def alignments(L, names):
    """every node row z* n1^r1 .. nk^rk o* of length L over the inner nodes n1 .. nk, r >= 1 -- r >= 0 for a '*' node --, and the
    row without the motif"""
    M = len(names)
    inner = list(range(1, M - 1))
    least = [0 if names[h] == "*" else 1 for h in inner]
    yield np.zeros(L, dtype=np.uint8)
    for m in range(sum(least), L + 1):
        for split in itertools.combinations_with_replacement(range(len(inner)), m - sum(least)):
            reps = list(least)
            for d in split:
                reps[d] += 1
            body = [h for h, n in zip(inner, reps) for _ in range(n)]
            if not body:
                continue
            for a in range(0, L - m + 1):
                yield np.array([0] * a + body + [M - 1] * (L - m - a), dtype=np.uint8)


def enumerated_profile(o, seq, qual):
    """(L, M) profile by brute force, or None for a sequence without a parse"""
    L = len(seq)
    names = o.hmm()["node"]
    M = len(names)
    Zo = o.derivation_logz(seq, qual, None, None)
    if not np.isfinite(Zo):
        return None
    prof = np.zeros((L, M))
    total, rows = 0.0, 0
    for h in alignments(L, names):
        rows += 1
        assert rows <= MAX_ROWS, rows
        w = np.exp(o.derivation_logz(seq, qual, None, h) - Zo)
        if w == 0.0:
            continue
        total += w
        prof[np.arange(L), h] += w
    assert abs(total - 1.0) <= 1e-12, total
    return prof


# ---- B: identities of the oracle's scan ---------------------------------------------------------------------------------------------

def bracket_partner(names):
    stack, partner = [], {}
    for k, c in enumerate(names):
        if c == "(":
            stack.append(k)
        elif c == ")":
            partner[k] = stack.pop()
    return partner


def assert_oracle_identities(o, seq, qual, prof, what=""):
    """sum over the inner nodes = exp(inner) of the scan; the mass of the nodes that own a theta row = the expected emission
    counts EN of that row, per base for a single-base row, the row's total for a pair row (against its ')' and its '(' node)"""
    hmm = o.hmm()
    names, tid, sizes = hmm["node"], hmm["theta_id"], hmm["theta_sizes"]
    M = len(names)
    sc = o.scan_seq(seq, qual)
    np.testing.assert_allclose(prof[:, 1:M - 1].sum(axis=1), np.exp(sc["inner"]), rtol=1e-8, atol=1e-10, err_msg="inner %s" % (what,))
    if o.flags & po.NO_PRF:
        return
    seq = np.asarray(seq)
    off = np.concatenate([[0], np.cumsum(sizes)])
    partner = bracket_partner(names)
    for r, size in enumerate(sizes):
        owners = [m for m in range(M) if tid[m] == r]
        en = sc["EN"][off[r]:off[r + 1]]
        if size == 4:
            got = np.array([prof[seq == b + 1][:, owners].sum() for b in range(4)])
            np.testing.assert_allclose(got, en, rtol=1e-8, atol=1e-10, err_msg="row %d %s" % (r, what))
        else:
            for m in owners:
                for node in (m, partner[m]):
                    np.testing.assert_allclose(prof[:, node].sum(), en.sum(), rtol=1e-8, atol=1e-10, err_msg="row %d node %d %s" % (r, node, what))


# ---- C: the definitions over the oracle's tables ------------------------------------------------------------------------------------

BP_TYPE = {(1, 4): 5, (2, 3): 1, (3, 2): 2, (3, 4): 3, (4, 1): 6, (4, 3): 4}   # rows N A C G U: AU 5, CG 1, GC 2, GU 3, UA 6, UG 4


def position_weights(qual):
    """ws[i] = log((0.01 + q_i) / (0.01 + mode(q))), the mode the last of the most frequent values"""
    qual = np.asarray(qual, dtype=np.int64)
    cnt = np.bincount(qual, minlength=94)
    mode = max(v for v in range(len(cnt)) if cnt[v] == cnt.max())
    return np.log((0.01 + qual[:-1]) / (0.01 + mode))


def table_profile(o, seq, qual, x, tau=0.1):
    """(L, M) profile from the oracle's inside / outside tables of the first (full-terminal) pass, or None without a parse: the
    five emitting rules of node_rules.h, each posterior out(parent) + weight + in(child) - Zo routed to the emitted node"""
    o.set_params(x)
    x = np.asarray(x, dtype=np.float64)
    seq = np.asarray(seq)
    L = len(seq)
    t = o.train_seq(seq, qual, tables=True)
    Zo = t["Zo"]
    if not np.isfinite(Zo):
        return None
    ins, outs, io_, oo = t["inside"], t["outside"], t["inside_o"], t["outside_o"]
    W = t["W"]
    hmm = o.hmm()
    names, tid, sizes = hmm["node"], hmm["theta_id"], hmm["theta_sizes"]
    M = len(names)
    states = [tuple(s) for s in hmm["state"]]
    sid = {s: k for k, s in enumerate(states)}
    lam = np.array([x[-2] if l == r else x[-1] for l, r in states])
    ne = bool(o.flags & po.NO_ENE)
    no_rss = bool(o.flags & po.NO_RSS)      # (no pair is kept then, and the oracle's filter is not run)
    kept = np.zeros((L + 1, W + 1), dtype=np.uint8) if no_rss else o.bpp(seq)[1]
    if not np.isfinite(t["Zari"]):
        oo = no_motif_outside_chain(o, seq, x, t, hmm, sid, kept, lam, ne)
    off = np.concatenate([[0], np.cumsum(sizes)])
    theta = [np.array(x[off[r]:off[r + 1]]) for r in range(len(sizes))]
    if o.flags & po.THETA_SOFTMAX:
        theta = [v - np.logaddexp.reduce(v) for v in theta]
    if o.flags & po.NO_PRF:
        theta = [np.zeros_like(v) for v in theta]
    ws = position_weights(qual)
    ltau = np.log(tau)
    P_, E_, M_, T2_, L_ = 0, 1, 2, 5, 6

    ty_of = np.zeros((5, 5), dtype=np.int64)
    for (bi, bj), ty in BP_TYPE.items():
        ty_of[bi, bj] = ty
    NEG = -np.inf

    # (the weights take position vectors)
    def single(node, pos):
        b = seq[pos].astype(np.int64)
        w = np.where(b > 0, theta[tid[node]][np.maximum(b, 1) - 1], 0.0) if tid[node] >= 0 else np.zeros(len(pos))
        return w + (ws[pos] if names[node] in ".()" else 0.0)

    def w_right(par, ch, pos):
        r = states[par][1]
        return single(r, pos) + (ltau if r == states[ch][1] and names[r] == "." else 0.0)

    def w_left(par, ch, pos):
        l = states[ch][0]
        return single(l, pos) + (ltau if l == states[par][0] and names[l] == "." else 0.0)

    def w_pair(par, ch, pi, pj):
        r, l = states[par][1], states[ch][0]
        if names[r] == ")":
            ty = ty_of[seq[pi].astype(np.int64), seq[pj].astype(np.int64)]
            w = np.where(ty > 0, theta[tid[r]][np.maximum(ty, 1) - 1], 0.0)
            w = w + (ws[pi] if names[l] in ".()" else 0.0) + ws[pj]
        else:
            w = single(l, pi) + single(r, pj)
        return w + (ltau if r == states[ch][1] and names[r] == ")" else 0.0)

    prof = np.zeros((L, M))

    def add(pos, node, v):
        """one term per position of pos (distinct positions)"""
        prof[pos, node] += np.exp(v - Zo)

    with np.errstate(invalid="ignore", over="ignore"):
        pos = np.arange(L)
        for s, (l, r) in enumerate(states):                                    # rule 8
            for s1 in hmm["right"][s]:
                add(pos, r, oo[pos + 1, s] + io_[pos, s1] + w_right(s, s1, pos))
        for d in range(1, (0 if no_rss else W) + 1):
            i = np.arange(0, L - d + 1)
            j = i + d
            if d >= 2:
                ik = i[kept[i, d] > 0]
                est = np.array([0.0 if ne else o.loop_energy(seq, int(a), int(a) + d - 1, int(a) + 1, int(a) + d - 2) for a in ik])
                stack_ok = (kept[ik + 1, d - 2] > 0) & np.isfinite(est)
                est = np.where(stack_ok, est, 0.0)
            for s, (l, r) in enumerate(states):
                if s in hmm["loop_state"]:                                     # L <- L
                    add(j - 1, r, ins[i, d, L_, s] + outs[i, d, L_, s])
                for s1 in hmm["right"][s]:                                     # 3a
                    add(j - 1, r, outs[i, d, T2_, s] + ins[i, d - 1, T2_, s1] + w_right(s, s1, j - 1))
                for sl in hmm["left"][s]:                                      # 5a
                    add(i, states[sl][0], outs[i, d, M_, s] + ins[i + 1, d - 1, M_, sl] + w_left(s, sl, i))
                if d >= 2 and len(ik):                                         # 1a, 1b
                    for sp in hmm["pair"][s]:
                        inner = np.logaddexp(ins[ik + 1, d - 2, E_, sp], np.where(stack_ok, ins[ik + 1, d - 2, P_, sp] + lam[s] * est, NEG))
                        v = outs[ik, d, P_, s] + w_pair(s, sp, ik, ik + d - 1) + inner
                        add(ik, states[sp][0], v)
                        add(ik + d - 1, r, v)
    assert not np.isnan(prof).any()
    return np.clip(prof, 0.0, 1.0)


def no_motif_outside_chain(o, seq, x, t, hmm, sid, kept, lam, ne):
    """outside_o of a sequence without any parse with the motif (Z(ari) = 0): the oracle's train schedule skips it and hands out
    no outside chain.  The only terminal left is (0, 0), a closed state: its chain runs backwards over that one state, rule 8 and
    rule 7 reversed, with the background row of theta and no position weight (ctx_check.no_motif_outside_chain, which also
    demands that no other state reaches the end of the inside chain; a motif prefix may, and weighs nothing here)."""
    L, W = len(seq), t["W"]
    assert hmm["node"][0] not in ".()" and hmm["theta_id"][0] == 0
    s0 = sid[(0, 0)]
    assert hmm["right"][s0] == [s0]
    th = np.array(x[:hmm["theta_sizes"][0]], dtype=np.float64)
    if o.flags & po.THETA_SOFTMAX:
        th = th - np.logaddexp.reduce(th)
    if o.flags & po.NO_PRF:
        th = np.zeros_like(th)
    oo = np.full((L + 1, len(sid)), -np.inf)
    oo[L, s0] = 0.0
    for i in range(L - 1, -1, -1):
        v = oo[i + 1, s0] + (th[seq[i] - 1] if seq[i] else 0.0)
        for d in range(1, W + 1):
            j = i + d
            if j <= L and kept[i, d]:
                tsc = 0.0 if ne else o.sum_ext_m(seq, i, j - 1, True)
                if np.isfinite(tsc):
                    v = np.logaddexp(v, oo[j, s0] + t["inside"][i, d, 0, s0] + lam[s0] * tsc)
        oo[i, s0] = v
    assert abs(oo[0, s0] - t["Zo"]) <= 1e-10 * max(1.0, abs(t["Zo"])), (oo[0, s0], t["Zo"])
    return oo


def no_parse_profile(L, M):
    prof = np.zeros((L, M))
    prof[:, 0] = 1.0
    return prof


# ---- the CPU driver of the product rule ---------------------------------------------------------------------------------------------

def driver():
    global _lib
    if _lib is None:
        srcs = [SRC] + _emul_build.SRCS[1:]
        deps = [SRC] + _emul_build.DEPS + [os.path.join(_emul_build.CSRC, f) for f in ("node_rules.h", "ctx_rules.h", "pair_rules.h")]
        if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in deps):
            subprocess.check_call(["g++", "-std=c++14", "-O2", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-o", LIB] + srcs)
        L = C.CDLL(LIB)
        dp, u8 = C.POINTER(C.c_double), C.POINTER(C.c_uint8)
        L.emu_create.restype = C.c_void_p
        L.emu_create.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int]
        L.emu_destroy.argtypes = [C.c_void_p]
        L.emu_last_error.restype = C.c_char_p
        L.emu_set_fast.argtypes = [C.c_void_p, C.c_int]
        L.emu_node_seq.argtypes = [C.c_void_p, dp, u8, C.c_int, u8, C.c_int, dp]
        _lib = L
    return _lib


class NodeDriver:
    LIN, LOG = 0, 1

    def __init__(self, pattern, par="~T2004~", max_span=50, max_iloop=30, min_bpp=1e-4, tau=0.1, flags=0, n_node=None):
        if par in ("~T2004~", "~A2007~"):
            par = po.energy_param_text(par)
        self.h = driver().emu_create(pattern.encode(), par.encode(), max_span, max_iloop, min_bpp, tau, flags)
        if not self.h:
            raise RuntimeError(driver().emu_last_error().decode())
        self.M = n_node

    def __del__(self):
        try:
            driver().emu_destroy(self.h)
        except Exception:
            pass

    def set_fast(self, on):
        driver().emu_set_fast(self.h, int(bool(on)))

    def profile(self, x, seq, qual, form=0):
        """((L, M) profile, the form that wrote it): form LIN hands a sequence on to LOG where Z leaves the double range or the
        sequence has no parse, as the engine does"""
        x = np.ascontiguousarray(x, dtype=np.float64)
        seq = np.ascontiguousarray(seq, dtype=np.uint8)
        qual = np.ascontiguousarray(qual, dtype=np.uint8)
        L, M = len(seq), self.M
        prof = np.full(max(M * L, 1), np.nan)
        dp, u8 = C.POINTER(C.c_double), C.POINTER(C.c_uint8)
        rc = driver().emu_node_seq(self.h, x.ctypes.data_as(dp), seq.ctypes.data_as(u8), L, qual.ctypes.data_as(u8), form,
                                   prof.ctypes.data_as(dp))
        if rc < 0:
            raise RuntimeError(driver().emu_last_error().decode())
        return prof[:M * L].reshape(L, M), rc
