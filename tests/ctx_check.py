"""Shared checks of the structural context profile: two references built from the oracle alone --
enumerated_profile (every structure over the kept cells, weighted by the oracle's own fixed-structure partition function and
classified from its dot-bracket) and table_profile (the definitions of ctx_rules.h in numpy over the oracle's inside / outside
tables) -- and the test-only CPU driver of the product rule (tests/ctx_emul.cpp)."""
import ctypes as C
import os
import subprocess

import numpy as np

from oracle import pyoracle as po
from tests.emul import build as _emul_build

LETTERS = "OLRHBIM"
MAX_STRUCTURES = 20000
HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "ctx_emul.cpp")
LIB = os.path.join(HERE, "libelemdp_ctx_emul.so")
_lib = None


# ---- the letters of one structure ------------------------------------------------------------------------------------------------

def classify(db):
    """rss letters of a dot-bracket: L / R on the bases of a pair; an unpaired base is O at the top level, else named after the
    loop its nearest enclosing pair closes: H without an inner pair, B with one inner pair and one empty side, I with one inner
    pair and bases on both sides, M with two or more inner pairs"""
    L = len(db)
    partner = [-1] * L
    stack = []
    for p, c in enumerate(db):
        if c == "(":
            stack.append(p)
        elif c == ")":
            a = stack.pop()
            partner[a], partner[p] = p, a
    assert not stack
    out = ["O"] * L

    def loop(a, b):
        """the loop closed by the pair (a, b)"""
        inner, unp = [], []
        p = a + 1
        while p < b:
            if partner[p] > p:
                inner.append((p, partner[p]))
                p = partner[p] + 1
            else:
                unp.append(p)
                p += 1
        if not inner:
            letter = "H"
        elif len(inner) == 1:
            k, l = inner[0]
            letter = "B" if (k == a + 1) != (l == b - 1) else "I"
        else:
            letter = "M"
        for p in unp:
            out[p] = letter
        out[a], out[b] = "L", "R"
        for k, l in inner:
            loop(k, l)

    p = 0
    while p < L:
        if partner[p] > p:
            loop(p, partner[p])
            p = partner[p] + 1
        else:
            p += 1
    return "".join(out)


def structures(kept, L, W, min_span=5):
    """every dot-bracket whose pairs are kept cells (i, d) of span min_span .. W (hairpins of at least 3 bases)"""
    ends = [[i + d for d in range(min_span, W + 1) if i + d <= L and kept[i, d]] for i in range(L + 1)]
    memo = {}

    def gen(a, b):
        """structures of [a, b) as tuples of pairs"""
        key = (a, b)
        if key in memo:
            return memo[key]
        res = [()]
        for i in range(a, b):
            for j in ends[i]:
                if j > b:
                    continue
                for inner in gen(i + 1, j - 1):
                    for rest in gen(j, b):
                        res.append(((i, j),) + inner + rest)
                        assert len(res) <= 50 * MAX_STRUCTURES
        memo[key] = res
        return res

    # (gen(a, b) lists the structures by their first pair: pairs (i, j) with everything left of i unpaired)
    out = []
    for prs in gen(0, L):
        s = ["."] * L
        for i, j in prs:
            s[i], s[j - 1] = "(", ")"
        out.append("".join(s))
    return out


def enumerated_profile(o, seq, qual):
    """(L, 7) profile by brute force, or None for a sequence without a parse"""
    L = len(seq)
    Zo = o.derivation_logz(seq, qual, None, None)
    if not np.isfinite(Zo):
        return None
    _, kept, _, _ = o.bpp(seq)
    W = kept.shape[1] - 1
    dbs = structures(kept, L, W)
    assert len(set(dbs)) == len(dbs)
    assert len(dbs) <= MAX_STRUCTURES, len(dbs)
    prof = np.zeros((L, 7))
    total = 0.0
    for db in dbs:
        w = np.exp(o.derivation_logz(seq, qual, db, None) - Zo)
        if w == 0.0:
            continue
        total += w
        for p, c in enumerate(classify(db)):
            prof[p, LETTERS.index(c)] += w
    assert abs(total - 1.0) <= 1e-12, total
    return prof


# ---- the definitions over the oracle's tables ---------------------------------------------------------------------------------------

def table_profile(o, seq, qual, x, bulge=True):
    """(L, 7) profile from the oracle's inside / outside tables of the first (full-terminal) pass, or None without a parse.  O is
    the complement of rule 7 (1 - the posterior that an exterior pair covers p), the other columns as ctx_rules.h states them.
    bulge False: B is left at NaN and I holds U - H (the item loop in Python is the expensive part)."""
    o.set_params(x)
    L = len(seq)
    t = o.train_seq(seq, qual, tables=True)
    Zo = t["Zo"]
    if not np.isfinite(Zo):
        return None
    if o.flags & po.NO_RSS:
        prof = np.zeros((L, 7))
        prof[:, 0] = 1.0
        return prof
    ins, outs, io_, oo = t["inside"], t["outside"], t["inside_o"], t["outside_o"]
    W = t["W"]
    hmm = o.hmm()
    states = [tuple(s) for s in hmm["state"]]
    sid = {s: k for k, s in enumerate(states)}
    loops = hmm["loop_state"]
    lam = [x[-2] if l == r else x[-1] for l, r in states]
    ne = bool(o.flags & po.NO_ENE)
    _, kept, _, _ = o.bpp(seq)
    C_ = min(W - 2 - 5, o.max_iloop_)
    P_, E_, L_ = 0, 1, 6

    lam = np.array(lam)
    loops = np.array(loops, dtype=int)
    # rule 7 / rule 2 splits (s; s2 = (s.l, h), s1 = (h, s.r)) and the rule-6c quadruples, as index arrays
    sp = np.array([(s, sid[(l, h)], sid[(h, r)]) for s, (l, r) in enumerate(states) for h in range(l, r + 1)
                   if (l, h) in sid and (h, r) in sid and hmm["reachable"][l][h] and hmm["reachable"][h][r]], dtype=int).reshape(-1, 3)
    qd = np.array(hmm["loop_loop"], dtype=int).reshape(-1, 4)

    def post(v):
        with np.errstate(invalid="ignore", over="ignore"):
            return float(np.nan_to_num(np.exp(v - Zo), nan=0.0).sum())

    if not np.isfinite(t["Zari"]):
        oo = no_motif_outside_chain(o, seq, x, t, hmm, sid, kept, lam, ne)

    Lp, R, U, H, B, X = (np.zeros(L) for _ in range(6))
    for i in range(L + 1):
        for d in range(1, W + 1):
            j = i + d
            if j > L:
                break
            if kept[i, d]:
                v = post(ins[i, d, P_, :] + outs[i, d, P_, :])
                Lp[i] += v
                R[j - 1] += v
                # rule 7: the pair (i, j) is exterior
                tsc = 0.0 if ne else o.sum_ext_m(seq, i, j - 1, True)
                if np.isfinite(tsc):
                    X[i:j] += post(oo[j, sp[:, 0]] + io_[i, sp[:, 1]] + ins[i, d, P_, sp[:, 2]] + lam[sp[:, 0]] * tsc)
            U[j - 1] += post(ins[i, d, L_, loops] + outs[i, d, L_, loops])
            e_ok = i > 0 and d + 2 <= W and kept[i - 1, d + 2]
            if not e_ok:
                continue
            tsc = 0.0 if ne else o.hairpin_energy(seq, i - 1, j)
            if np.isfinite(tsc):
                H[i:j] += post(outs[i, d, E_, loops] + lam[loops] * tsc + ins[i, d, L_, loops])
            if not bulge:
                continue
            for l in range(j, max(i, j - C_) - 1, -1):
                for k in range(i, min(l, i + C_ - (j - l)) + 1):
                    if (k == i) == (l == j) or l - k < 1 or not kept[k, l - k]:
                        continue
                    tsc = 0.0 if ne else o.loop_energy(seq, i - 1, j, k, l - 1)
                    if not np.isfinite(tsc):
                        continue
                    w = post(outs[i, d, E_, qd[:, 0]] + lam[qd[:, 0]] * tsc + ins[k, l - k, P_, qd[:, 1]] + ins[i, k - i, L_, qd[:, 2]]
                             + ins[l, j - l, L_, qd[:, 3]])
                    B[i:k] += w
                    B[l:j] += w
    prof = np.zeros((L, 7))
    prof[:, 0] = 1.0 - X
    prof[:, 1], prof[:, 2], prof[:, 3] = Lp, R, H
    prof[:, 4] = B if bulge else np.nan
    prof[:, 5] = np.maximum(0.0, U - H - (B if bulge else 0.0))
    prof[:, 6] = np.maximum(0.0, 1.0 - Lp - R - U - prof[:, 0])
    return prof


def no_motif_outside_chain(o, seq, x, t, hmm, sid, kept, lam, ne):
    """outside_o of a sequence without any parse with the motif (Z(ari) = 0): the oracle's train schedule skips it and hands out
    its band tables only.  Every parse left keeps every state at (0, 0), whose emissions carry the background row of theta and no
    position weight, so the exterior chain runs backwards over that one state: rule 8 and rule 7 reversed."""
    L, W = len(seq), t["W"]
    assert hmm["node"][0] not in ".()" and hmm["theta_id"][0] == 0
    s0 = sid[(0, 0)]
    assert all(not np.isfinite(t["inside_o"][L, s]) for s in range(len(sid)) if s != s0)
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


def ctx_oracle(pattern, W=50, C=30, min_bpp=1e-4, tau=0.1, flags=0, par_text=None):
    o = po.make_oracle(pattern, W, C, min_bpp=min_bpp, tau=tau, flags=flags, par_text=par_text)
    o.max_iloop_ = C
    return o


def ctx_oracle_from_model(path):
    o, x = po.oracle_from_model(path)
    o.max_iloop_ = po.read_model(path)["max_iloop"]
    return o, x


# ---- the CPU driver of the product rule ---------------------------------------------------------------------------------------------

def driver():
    global _lib
    if _lib is None:
        srcs = [SRC] + _emul_build.SRCS[1:]
        deps = [SRC] + _emul_build.DEPS + [os.path.join(_emul_build.CSRC, f) for f in ("ctx_rules.h", "pair_rules.h")]
        if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in deps):
            subprocess.check_call(["g++", "-std=c++14", "-O2", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-o", LIB] + srcs)
        L = C.CDLL(LIB)
        dp, u8 = C.POINTER(C.c_double), C.POINTER(C.c_uint8)
        L.emu_create.restype = C.c_void_p
        L.emu_create.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int]
        L.emu_destroy.argtypes = [C.c_void_p]
        L.emu_last_error.restype = C.c_char_p
        L.emu_set_fast.argtypes = [C.c_void_p, C.c_int]
        L.emu_ctx_seq.argtypes = [C.c_void_p, dp, u8, C.c_int, u8, C.c_int, dp]
        _lib = L
    return _lib


class CtxDriver:
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

    def profile(self, x, seq, qual, form=0):
        """((L, 7) profile, the form that wrote it): form LIN hands a sequence on to LOG where Z leaves the double range or the
        sequence has no parse, as the engine does"""
        x = np.ascontiguousarray(x, dtype=np.float64)
        seq = np.ascontiguousarray(seq, dtype=np.uint8)
        qual = np.ascontiguousarray(qual, dtype=np.uint8)
        L = len(seq)
        prof = np.full(max(7 * L, 1), np.nan)
        dp, u8 = C.POINTER(C.c_double), C.POINTER(C.c_uint8)
        rc = driver().emu_ctx_seq(self.h, x.ctypes.data_as(dp), seq.ctypes.data_as(u8), L, qual.ctypes.data_as(u8), form,
                                  prof.ctypes.data_as(dp))
        if rc < 0:
            raise RuntimeError(driver().emu_last_error().decode())
        return prof[:7 * L].reshape(L, 7), rc


def exterior_only(L):
    prof = np.zeros((L, 7))
    prof[:, 0] = 1.0
    return prof


def assert_profile(got, ref, what="", cols=range(7)):
    """the project's `unpaired` tolerances"""
    cols = list(cols)
    np.testing.assert_allclose(got[:, cols], ref[:, cols], rtol=1e-8, atol=1e-10, err_msg=str(what))


def no_parse_inputs(x, hmm):
    """(x', poly-A, a sequence without A, their qualities): x with log-probability -inf for base A in every single-base row of
    theta, under which poly-A has no parse at all (Z(ari, nasi) = 0: every parse emits every base) and a sequence of C, G and U
    keeps all of its parses"""
    xx = np.array(x, dtype=np.float64)
    off = 0
    for size in hmm["theta_sizes"]:
        if size == 4:
            xx[off] = -np.inf
        off += size
    rng = np.random.default_rng(17)
    seqs = [np.ones(30, dtype=np.uint8), rng.integers(2, 5, size=40).astype(np.uint8)]
    quals = [np.full(len(s) + 1, 10, dtype=np.uint8) for s in seqs]
    quals[0][-1] = 0
    return xx, seqs, quals
