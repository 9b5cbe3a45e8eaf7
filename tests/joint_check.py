"""Shared checks of the joint node-by-context posteriors.  Two references built from the oracle alone:
A. enumerated_joint -- every structure of ctx_check.structures times every node row of node_check.alignments, each weighted by
   the oracle's own derivation_logz and classified by ctx_check.classify;
B. table_joint -- the definitions of joint_rules.h in numpy over the oracle's inside / outside tables: the five routed parts
   with the emission weights restated as node_check.table_profile restates them, the hairpin and bulge chains with the bulge
   items enumerated as ctx_check.table_profile enumerates them;
and the test-only CPU driver of the product rule (tests/joint_emul.cpp)."""
import ctypes as C
import os
import subprocess

import numpy as np

from oracle import pyoracle as po
from tests import ctx_check as cc
from tests import node_check as nc
from tests.emul import build as _emul_build

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "joint_emul.cpp")
LIB = os.path.join(HERE, "libelemdp_joint_emul.so")
O_, L_, R_, H_, B_, I_, M_ = range(7)        # CtxCol order
PARTS_ALL, PART_SEED_H, PART_SEED_B, PART_CHAIN = 7, 1, 2, 4
_lib = None

joint_oracle = cc.ctx_oracle
joint_oracle_from_model = cc.ctx_oracle_from_model


def assert_joint(got, ref, what=""):
    """the project's `unpaired` tolerances, entry by entry"""
    np.testing.assert_allclose(got, ref, rtol=1e-8, atol=1e-10, err_msg=str(what))


def counts_of(prof, seq):
    """(M, 7, 5) expected emission counts of an (L, M, 7) profile: positions by base code N A C G U"""
    seq = np.asarray(seq)
    return np.stack([prof[seq == b].sum(axis=0) for b in range(5)], axis=-1)


def no_parse_joint(L, M):
    prof = np.zeros((L, M, 7))
    prof[:, 0, O_] = 1.0
    return prof


# ---- the enumerated cases, shared by the CPU and the GPU tests (each reference is computed once per process) ---------------------------

PAR = "~T2004~"
# (pattern, L, flags, min_bpp): three patterns, with and without energies, min_bpp 0 and 1e-4 -- sizes the pruned enumeration does
# in a few seconds each -- and one case of 16 bases, the shortest at which a node of the pattern emits a base of a multi-branch loop
# (the M letter on the nodes 1 .. M-2)
TINY = [("((.*.))", 14), ("(.*)", 14), (".(.*).", 13)]
CASES = [(p, L, f, b) for p, L in TINY for f in (0, po.NO_ENE) for b in (0.0, 1e-4)] + [("(.*)", 16, po.NO_ENE, 0.0)]
_refs = {}


def case_id(c):
    return "%s-%d-%d-%g" % c


def joint_params(eng):
    """perturbed initial parameters with lambda = (1.0, 0.7)"""
    x = eng.initial_params(1.0)
    x[:-2] += np.linspace(-0.3, 0.3, len(x) - 2)
    x[-2:] = (1.0, 0.7)
    return x


def tiny_inputs(case):
    from rnaelem_amd import api, synth
    pattern, L, flags, min_bpp = case
    x = joint_params(api.Engine(pattern, PAR, 50, 30, min_bpp, 0.1, flags, 0))
    (s,), (q,) = synth.synth_batch(1, L, seed=100 + L)
    return x, s, q


def tiny_reference(case):
    """(x, seq, qual, oracle, enumerated joint) of an enumerated case"""
    if case not in _refs:
        pattern, _, flags, min_bpp = case
        x, s, q = tiny_inputs(case)
        o = joint_oracle(pattern, 50, 30, min_bpp=min_bpp, flags=flags)
        o.set_params(x)
        _refs[case] = (x, s, q, o, enumerated_joint(o, s, q))
    return _refs[case]


# ---- A: enumeration ------------------------------------------------------------------------------------------------------------------

def enumerated_joint(o, seq, qual):
    """(L, M, 7) joint by brute force, or None for a sequence without a parse.  The weight of each structure alone and of each
    node row alone comes first; only the live ones are combined, and a row only with the structures whose brackets fit it."""
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
    letters = [np.array([cc.LETTERS.index(c) for c in cc.classify(db)]) for db in dbs]
    # a '(' node is emitted as the left base of a pair and a ')' node as the right base: a row meets only the structures that
    # have a '(' and a ')' there (were that wrong, the total below would fall short of 1)
    chars = np.array([list(db) for db in dbs]).reshape(len(dbs), L)
    is_open = np.array([c == "(" for c in names])
    is_close = np.array([c == ")" for c in names])
    prof = np.zeros((L, M, 7))
    pos = np.arange(L)
    total = 0.0
    for h in rows:
        fits = np.all((chars == "(") | ~is_open[h], axis=1) & np.all((chars == ")") | ~is_close[h], axis=1)
        for k in np.nonzero(fits)[0]:
            w = np.exp(o.derivation_logz(seq, qual, dbs[k], h) - Zo)
            if w == 0.0:
                continue
            total += w
            prof[pos, h, letters[k]] += w
    assert abs(total - 1.0) <= 1e-12, total
    return prof


# ---- B: the definitions over the oracle's tables ------------------------------------------------------------------------------------

def table_joint(o, seq, qual, x, tau=0.1, parts=PARTS_ALL):
    """(L, M, 7) joint from the oracle's inside / outside tables of the first (full-terminal) pass, or None without a parse.
    parts: the terms of G that take part (PART_* bits), for the tests that show that a dropped term is seen."""
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
    S = len(states)
    sid = {s: k for k, s in enumerate(states)}
    lam = np.array([x[-2] if l == r else x[-1] for l, r in states])
    ne = bool(o.flags & po.NO_ENE)
    no_rss = bool(o.flags & po.NO_RSS)
    kept = np.zeros((L + 1, W + 1), dtype=np.uint8) if no_rss else o.bpp(seq)[1]
    if not np.isfinite(t["Zari"]):
        oo = nc.no_motif_outside_chain(o, seq, x, t, hmm, sid, kept, lam, ne)
    off = np.concatenate([[0], np.cumsum(sizes)])
    theta = [np.array(x[off[r]:off[r + 1]]) for r in range(len(sizes))]
    if o.flags & po.THETA_SOFTMAX:
        theta = [v - np.logaddexp.reduce(v) for v in theta]
    if o.flags & po.NO_PRF:
        theta = [np.zeros_like(v) for v in theta]
    ws = nc.position_weights(qual)
    ltau = np.log(tau)
    tP, tE, tM, t2, tL = 0, 1, 2, 5, 6
    ty_of = np.zeros((5, 5), dtype=np.int64)
    for (bi, bj), ty in nc.BP_TYPE.items():
        ty_of[bi, bj] = ty
    NEG = -np.inf

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

    prof = np.zeros((L, M, 7))
    U = np.zeros((L, M))                                                       # the L <- L part of N(p, m)

    def add(pos, node, col, v):
        prof[pos, node, col] += np.exp(v - Zo)

    loops = list(hmm["loop_state"])
    is_loop = np.zeros(S, dtype=bool)
    is_loop[loops] = True
    with np.errstate(invalid="ignore", over="ignore"):
        pos = np.arange(L)
        for s, (l, r) in enumerate(states):                                    # rule 8
            for s1 in hmm["right"][s]:
                add(pos, r, O_, oo[pos + 1, s] + io_[pos, s1] + w_right(s, s1, pos))
        for d in range(1, (0 if no_rss else W) + 1):
            i = np.arange(0, L - d + 1)
            j = i + d
            if d >= 2:
                ik = i[kept[i, d] > 0]
                est = np.array([0.0 if ne else o.loop_energy(seq, int(a), int(a) + d - 1, int(a) + 1, int(a) + d - 2) for a in ik])
                stack_ok = (kept[ik + 1, d - 2] > 0) & np.isfinite(est)
                est = np.where(stack_ok, est, 0.0)
            for s, (l, r) in enumerate(states):
                if is_loop[s]:                                                 # L <- L
                    U[j - 1, r] += np.exp(ins[i, d, tL, s] + outs[i, d, tL, s] - Zo)
                for s1 in hmm["right"][s]:                                     # 3a
                    add(j - 1, r, M_, outs[i, d, t2, s] + ins[i, d - 1, t2, s1] + w_right(s, s1, j - 1))
                for sl in hmm["left"][s]:                                      # 5a
                    add(i, states[sl][0], M_, outs[i, d, tM, s] + ins[i + 1, d - 1, tM, sl] + w_left(s, sl, i))
                if d >= 2 and len(ik):                                         # 1a, 1b
                    for sp in hmm["pair"][s]:
                        inner = np.logaddexp(ins[ik + 1, d - 2, tE, sp], np.where(stack_ok, ins[ik + 1, d - 2, tP, sp] + lam[s] * est, NEG))
                        v = outs[ik, d, tP, s] + w_pair(s, sp, ik, ik + d - 1) + inner
                        add(ik, states[sp][0], L_, v)
                        add(ik + d - 1, r, R_, v)

        if not no_rss:
            # ---- the seeds: seed[kind][i, d, s]
            seed = np.full((2, L + 1, W + 1, S), NEG)
            C_ = min(W - 2 - 5, o.max_iloop_)
            qd = np.array(hmm["loop_loop"], dtype=int).reshape(-1, 4)
            for i in range(1, L + 1):
                for d in range(1, W + 1):
                    j = i + d
                    if j > L:
                        break
                    if not (d + 2 <= W and kept[i - 1, d + 2]):                # e_ok
                        continue
                    if parts & PART_SEED_H:
                        tsc = 0.0 if ne else o.hairpin_energy(seq, i - 1, j)
                        if np.isfinite(tsc):
                            seed[0, i, d, loops] = outs[i, d, tE, loops] + lam[loops] * tsc
                    if not (parts & PART_SEED_B) or not len(qd):
                        continue
                    for l in range(j, max(i, j - C_) - 1, -1):
                        for k in range(i, min(l, i + C_ - (j - l)) + 1):
                            if (k == i) == (l == j) or l - k < 1 or not kept[k, l - k]:
                                continue
                            tsc = 0.0 if ne else o.loop_energy(seq, i - 1, j, k, l - 1)
                            if not np.isfinite(tsc):
                                continue
                            # (the run's own in(L) factor is left out: qd[:, 2] for the left run [i, k), qd[:, 3] for the right run [l, j))
                            base = outs[i, d, tE, qd[:, 0]] + lam[qd[:, 0]] * tsc + ins[k, l - k, tP, qd[:, 1]]
                            if l == j:
                                np.logaddexp.at(seed[1, i, k - i], qd[:, 2], base + ins[l, 0, tL, qd[:, 3]])
                            else:
                                np.logaddexp.at(seed[1, l, j - l], qd[:, 3], base + ins[i, 0, tL, qd[:, 2]])
            # ---- the chains, row by row, and the sums by emitted node
            tr = [(par, ch) for par in loops for ch in hmm["right"][par] if is_loop[ch]]
            tpar = np.array([a for a, _ in tr], dtype=int)
            tch = np.array([b for _, b in tr], dtype=int)
            allpos = np.arange(L)
            wtr = np.stack([w_right(a, b, allpos) for a, b in tr], axis=1) if tr else np.zeros((L, 0))   # [pos, transition]
            r_of = np.array([states[s][1] for s in range(S)])
            for i in range(L):
                dmax = min(W, L - i)
                prev = np.full((2, S), NEG)
                for d in range(dmax, 0, -1):
                    j = i + d
                    G = seed[:, i, d, :].copy()
                    if (parts & PART_CHAIN) and d < dmax and len(tr):
                        for c in range(2):
                            np.logaddexp.at(G[c], tch, prev[c, tpar] + wtr[j])
                    live = is_loop & np.isfinite(ins[i, d, tL, :])
                    G[:, ~live] = NEG
                    for c, col in ((0, H_), (1, B_)):
                        v = np.exp(ins[i, d, tL, live] + G[c, live] - Zo)
                        np.add.at(prof[j - 1, :, col], r_of[live], np.nan_to_num(v, nan=0.0))
                    prev = G
    assert not np.isnan(prof).any()
    prof = np.clip(prof, 0.0, 1.0)
    prof[:, :, I_] = np.clip(U - prof[:, :, H_] - prof[:, :, B_], 0.0, 1.0)
    return prof


# ---- the CPU driver of the product rule ---------------------------------------------------------------------------------------------

def driver():
    global _lib
    if _lib is None:
        srcs = [SRC] + _emul_build.SRCS[1:]
        deps = [SRC] + _emul_build.DEPS + [os.path.join(_emul_build.CSRC, f) for f in ("joint_rules.h", "node_rules.h", "ctx_rules.h", "pair_rules.h")]
        if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in deps):
            subprocess.check_call(["g++", "-std=c++14", "-O2", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-o", LIB] + srcs)
        L = C.CDLL(LIB)
        dp, u8 = C.POINTER(C.c_double), C.POINTER(C.c_uint8)
        L.emu_create.restype = C.c_void_p
        L.emu_create.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int]
        L.emu_destroy.argtypes = [C.c_void_p]
        L.emu_last_error.restype = C.c_char_p
        L.emu_set_fast.argtypes = [C.c_void_p, C.c_int]
        L.emu_joint_seq.argtypes = [C.c_void_p, dp, u8, C.c_int, u8, C.c_int, C.c_int, dp, dp]
        _lib = L
    return _lib


class JointDriver:
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

    def joint(self, x, seq, qual, form=0, parts=PARTS_ALL):
        """((L, M, 7) profile, (M, 7, 5) counts, the form that wrote them): form LIN hands a sequence on to LOG where Z leaves the
        double range or the sequence has no parse, as the engine does"""
        x = np.ascontiguousarray(x, dtype=np.float64)
        seq = np.ascontiguousarray(seq, dtype=np.uint8)
        qual = np.ascontiguousarray(qual, dtype=np.uint8)
        L, M = len(seq), self.M
        prof = np.full(max(7 * M * L, 1), np.nan)
        counts = np.full(35 * M, np.nan)
        dp, u8 = C.POINTER(C.c_double), C.POINTER(C.c_uint8)
        rc = driver().emu_joint_seq(self.h, x.ctypes.data_as(dp), seq.ctypes.data_as(u8), L, qual.ctypes.data_as(u8), form, parts,
                                    prof.ctypes.data_as(dp), counts.ctypes.data_as(dp))
        if rc < 0:
            raise RuntimeError(driver().emu_last_error().decode())
        return prof[:7 * M * L].reshape(L, M, 7), counts.reshape(M, 7, 5), rc
