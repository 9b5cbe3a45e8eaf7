"""References for the hard structure constraints, independent of constraint_rules.h: the pair mask by
brute force (pair by pair, explicit loops over the forced pairs), the test whether a dot-bracket satisfies a string, random strings,
and the constrained ensemble by enumeration with the oracle (ctx_check.structures weighted by derivation_logz, restricted to the
structures that satisfy the string and renormalised)."""
import numpy as np

from tests import ctx_check as cc

ALPHABET = ".x|<>()"
PAIRING = {(1, 4), (4, 1), (2, 3), (3, 2), (3, 4), (4, 3)}      # codes N A C G U: AU UA CG GC GU UG


def forced_pairs(cons):
    """[(a, b)] of the '(' ')' of a string, 0-based bases; ValueError for an unbalanced string or an unknown character"""
    stack, out = [], []
    for p, c in enumerate(cons):
        if c not in ALPHABET:
            raise ValueError("unknown character %r at %d" % (c, p))
        if c == "(":
            stack.append(p)
        elif c == ")":
            if not stack:
                raise ValueError("unbalanced at %d" % p)
            out.append((stack.pop(), p))
    if stack:
        raise ValueError("unbalanced at %d" % stack[-1])
    return out


def canonical(seq, L, W, min_span, i, j):
    """may bases i < j pair by sequence and span alone"""
    d = j - i + 1
    return min_span <= d <= W and j < L and (int(seq[i]), int(seq[j])) in PAIRING


def apply(kept, seq, cons, L, W, min_span=5):
    """(kept_out[(L+1), (W+1)], unp[L+1]) of one sequence: the filter's pairs the string allows, and the forced pairs"""
    assert len(cons) == L and kept.shape == (L + 1, W + 1)
    forced = forced_pairs(cons)
    partner = {}
    for a, b in forced:
        if not canonical(seq, L, W, min_span, a, b):
            raise ValueError("forced pair (%d, %d) is not canonical" % (a, b))
        partner[a], partner[b] = b, a
    out = np.zeros_like(kept)
    for i in range(L + 1):
        for d in range(W + 1):
            if d < 1 or i + d > L:
                out[i, d] = kept[i, d]          # (no cell: the bit stays)
                continue
            r = i + d - 1
            if not kept[i, d]:
                continue
            if cons[i] == "x" or cons[r] == "x":
                continue
            if not (cons[i] in ".|<" or partner.get(i) == r):
                continue
            if not (cons[r] in ".|>" or partner.get(r) == i):
                continue
            crossing = False
            for a, b in forced:
                if a < i < b < r or i < a < r < b:
                    crossing = True
            if not crossing:
                out[i, d] = 1
    for a, b in forced:
        out[a, b - a + 1] = 1
    unp = np.array([1 if c in ".x" else 0 for c in cons] + [1], dtype=np.uint8)
    return out, unp


def partners_of(db):
    stack, partner = [], [-1] * len(db)
    for p, c in enumerate(db):
        if c == "(":
            stack.append(p)
        elif c == ")":
            a = stack.pop()
            partner[a], partner[p] = p, a
    return partner


def satisfies(db, cons):
    """does the dot-bracket db satisfy the constraint string?"""
    partner = partners_of(db)
    want = dict()
    for a, b in forced_pairs(cons):
        want[a], want[b] = b, a
    for p, c in enumerate(cons):
        q = partner[p]
        if c == "x" and q >= 0:
            return False
        if c == "|" and q < 0:
            return False
        if c == "<" and not q > p:
            return False
        if c == ">" and not 0 <= q < p:
            return False
        if c in "()" and q != want[p]:
            return False
    return True


def letters_to_db(rss):
    """the dot-bracket of a string of structure letters (O L R H B I M)"""
    return "".join("(" if c == "L" else ")" if c == "R" else "." for c in rss)


def random_string(rng, seq, L, W, min_span=5, p_forced=0.5, kept=None, p_single=0.3):
    """a random constraint string of L characters: a few nested or adjacent forced pairs (canonical ones; with kept, pairs of
    that mask), then the single-base characters on the rest"""
    cons = ["."] * L
    forced = []
    if rng.random() < p_forced:
        cands = [(i, j) for i in range(L) for j in range(i + min_span - 1, min(L, i + W)) if canonical(seq, L, W, min_span, i, j)
                 and (kept is None or kept[i, j - i + 1])]
        rng.shuffle(cands)
        for i, j in cands[:8]:
            if len(forced) >= 3:
                break
            if all((j < a or i > b or (i < a and b < j) or (a < i and j < b)) for a, b in forced):
                forced.append((i, j))
                cons[i], cons[j] = "(", ")"
    for p in range(L):
        if cons[p] == "." and rng.random() < p_single:
            cons[p] = "x|<>"[rng.integers(4)]
    return "".join(cons)


def string_from_structure(rng, db, p_force=0.3, p_mark=0.3, p_x=0.2):
    """a constraint string the dot-bracket db satisfies: some of its pairs forced, on others '<' / '|' at the 5' base and '>' / '|'
    at the 3' base, 'x' on some of its unpaired bases"""
    cons = ["."] * len(db)
    for a, b in enumerate(partners_of(db)):
        if b < 0:
            if rng.random() < p_x:
                cons[a] = "x"
        elif b > a:
            u = rng.random()
            if u < p_force:
                cons[a], cons[b] = "(", ")"
            elif u < p_force + p_mark:
                cons[a], cons[b] = "<|"[rng.integers(2)], ">|"[rng.integers(2)]
    return "".join(cons)


LETTERS = cc.LETTERS


def enumerated(o, seq, qual, cons, dbs=None, U=6):
    """The constrained ensemble of one sequence by brute force: dict(lnZ, P[(L+1), (W+1)], unpaired[L], ctx[L, 7], access[L, U] (the
    probability that the bases p .. p + w are all unpaired, NaN where the window runs off the end), n_all, n_sat, n_dropped), or
    dict(lnZ=-inf, n_all, n_sat) when no structure of positive weight satisfies the string.  lnZ is that of the terminal set the
    oracle's derivation_logz sums (every parse of the sequence)."""
    L = len(seq)
    _, kept, _, _ = o.bpp(seq)
    W = kept.shape[1] - 1
    # (a forced pair the filter dropped comes back: enumerate over the constrained mask)
    kept_c, _ = apply(np.asarray(kept, dtype=np.uint8), seq, cons, L, W)
    all_dbs = cc.structures(kept, L, W) if dbs is None else dbs
    sat = [db for db in cc.structures(kept_c, L, W) if satisfies(db, cons)]
    assert len(sat) <= cc.MAX_STRUCTURES
    n_dropped = sum(1 for db in all_dbs if not satisfies(db, cons))
    lw = np.array([o.derivation_logz(seq, qual, db, None) for db in sat]) if sat else np.zeros(0)
    out = dict(n_all=len(all_dbs), n_sat=len(sat), n_dropped=n_dropped)
    live = np.isfinite(lw)
    if not live.any():
        out["lnZ"] = -np.inf
        return out
    top = lw[live].max()
    lnZ = top + np.log(np.exp(lw[live] - top).sum())
    P = np.zeros((L + 1, W + 1))
    unpaired = np.zeros(L)
    ctx = np.zeros((L, 7))
    access = np.zeros((L, U))
    for p in range(L):
        access[p, max(0, L - p):] = np.nan
    for db, l in zip(sat, lw):
        if not np.isfinite(l):
            continue
        w = np.exp(l - lnZ)
        partner = partners_of(db)
        for p, c in enumerate(cc.classify(db)):
            ctx[p, LETTERS.index(c)] += w
            if partner[p] > p:
                P[p, partner[p] - p + 1] += w
            elif partner[p] < 0:
                unpaired[p] += w
                for u in range(min(U, L - p)):
                    if partner[p + u] >= 0:
                        break
                    access[p, u] += w
    out.update(lnZ=lnZ, P=P, unpaired=unpaired, ctx=ctx, access=access, dbs=[db for db, l in zip(sat, lw) if np.isfinite(l)])
    return out


def live_rows(o, seq, qual):
    """the node rows of node_check.alignments that carry weight in the free ensemble (row 0 of the result list is the row without
    the motif when it is live: its first entry says so), or None where the sequence has more than node_check.MAX_ROWS rows"""
    from tests import node_check as nc
    names = o.hmm()["node"]
    rows = []
    for n, h in enumerate(nc.alignments(len(seq), names)):
        if n >= nc.MAX_ROWS:
            return None
        if np.isfinite(o.derivation_logz(seq, qual, None, h)):
            rows.append((n == 0, h))
    return rows


def node_reference(o, seq, qual, e, rows):
    """adds to the reference e of enumerated() the (L, M) node profile, ln Z(ari) and ln Z(nasi) of the constrained ensemble: every
    satisfying structure of weight with every live node row, weighted by derivation_logz(db, row); Z(nasi) is the share of the
    row without the motif, Z(ari) that of the others"""
    L, M = len(seq), len(o.hmm()["node"])
    prof = np.zeros((L, M))
    ari, nasi = [], []
    for db in e["dbs"]:
        for plain, h in rows:
            l = o.derivation_logz(seq, qual, db, h)
            if not np.isfinite(l):
                continue
            prof[np.arange(L), h] += np.exp(l - e["lnZ"])
            (nasi if plain else ari).append(l)
    assert abs(prof.sum(axis=1) - 1.0).max() <= 1e-10, abs(prof.sum(axis=1) - 1.0).max()
    e.update(node=prof, Zari=np.logaddexp.reduce(ari) if ari else -np.inf, Znasi=np.logaddexp.reduce(nasi) if nasi else -np.inf)


# ---- the enumerated cases, shared by the CPU and the GPU tests (each reference is computed once per process) ---------------------------

# the two sequences of the design note with their strings and the number of structures that satisfy each (0: unsatisfiable)
QUOTED = [
    (("(.*)", 16, 0, 0.0), "GGGACUUCGGUCCCAG", 534,
     [("...x....x.......", 317), ("|...............", 284), ("(............)..", 83), ("..(........)....", 48),
      (".x(...xx...)|...", 8), ("((..........)).x", 22), ("...|............", 84)]),
    (("(.*)", 20, 4, 0.0), "GGCGAAAGCCAGGGAAACCC", 994,
     [("....xxxx............", 676), ("|..................|", 305), ("(..................)", 235), ("..........|.........", 0)]),
]
_cases = {}


def case_strings(o, seq, n=2, tries=200, seed0=0):
    """n strings for one sequence of an enumerated case, drawn with fixed seeds: each keeps at least 2 and drops at least 2 of the
    structures over the oracle's mask; forced pairs are pairs of that mask"""
    L = len(seq)
    _, kept, _, _ = o.bpp(seq)
    W = kept.shape[1] - 1
    dbs = cc.structures(kept, L, W)
    out = []
    for seed in range(tries):
        rng = np.random.default_rng(seed0 + seed)
        cons = random_string(rng, seq, L, W, kept=kept, p_single=0.12, p_forced=0.5 if len(out) else 1.0)
        n_sat = sum(1 for db in dbs if satisfies(db, cons))
        if n_sat >= 2 and len(dbs) - n_sat >= 2 and cons not in out:
            out.append(cons)
            if len(out) == n:
                return out
    raise AssertionError("no strings found")


def enumerated_cases():
    """[(case, x, seq, qual, [(string, reference of enumerated() and, within node_check.MAX_ROWS rows, node_reference())])]:
    joint_check.CASES with strings of case_strings, and QUOTED; the cases are worked out side by side, each with an oracle of its own"""
    if "all" in _cases:
        return _cases["all"]
    from concurrent.futures import ThreadPoolExecutor
    from rnaelem_amd import api, io
    from tests import joint_check as jc
    from tests.pair_check import n_workers

    def with_nodes(o, s, q, refs):
        rows = live_rows(o, s, q)
        for c, e in refs:
            if rows is not None and np.isfinite(e["lnZ"]):
                node_reference(o, s, q, e, rows)
        return refs

    def tiny(job):
        n, case = job
        pattern, _, flags, min_bpp = case
        x, s, q = jc.tiny_inputs(case)
        o = jc.joint_oracle(pattern, 50, 30, min_bpp=min_bpp, flags=flags)
        o.set_params(x)
        return case, x, s, q, with_nodes(o, s, q, [(c, enumerated(o, s, q, c)) for c in case_strings(o, s, seed0=1000 * n)])

    def quoted(job):
        case, text, n_all, strings = job
        pattern, L, flags, min_bpp = case
        x = jc.joint_params(api.Engine(pattern, jc.PAR, 50, 30, min_bpp, 0.1, flags, 0))
        s = io.encode_seq(text)
        q = np.full(L + 1, 10, dtype=np.uint8)
        o = jc.joint_oracle(pattern, 50, 30, min_bpp=min_bpp, flags=flags)
        o.set_params(x)
        refs = []
        for c, n_sat in strings:
            e = enumerated(o, s, q, c)
            assert (e["n_all"], e["n_sat"]) == (n_all, n_sat), (text, c, e["n_all"], e["n_sat"])
            refs.append((c, e))
        return case, x, s, q, with_nodes(o, s, q, refs)

    with ThreadPoolExecutor(max_workers=n_workers()) as ex:
        a = ex.map(quoted, QUOTED)          # (the longest first)
        b = ex.map(tiny, list(enumerate(jc.CASES)))
        out = list(b) + list(a)
    _cases["all"] = out
    return out


# ---- the CPU driver of the product rules under a constraint (tests/constraint_emul.cpp) -------------------------------------------------

_lib = None


def driver():
    global _lib
    if _lib is None:
        import ctypes as C
        import os
        import subprocess
        from tests.emul import build as eb
        here = os.path.dirname(os.path.abspath(__file__))
        src, lib = os.path.join(here, "constraint_emul.cpp"), os.path.join(here, "libelemdp_constraint_emul.so")
        deps = [src] + eb.DEPS + [os.path.join(eb.CSRC, f) for f in ("ctx_rules.h", "pair_rules.h", "constraint_rules.h", "live_blocks.h")]
        if not os.path.exists(lib) or any(os.path.getmtime(d) > os.path.getmtime(lib) for d in deps):
            subprocess.check_call(["g++", "-std=c++14", "-O2", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-o", lib, src] + eb.SRCS[1:])
        L = C.CDLL(lib)
        dp, u8 = C.POINTER(C.c_double), C.POINTER(C.c_uint8)
        L.emu_create.restype = C.c_void_p
        L.emu_create.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int]
        L.emu_destroy.argtypes = [C.c_void_p]
        L.emu_last_error.restype = C.c_char_p
        L.emu_set_fast.argtypes = [C.c_void_p, C.c_int]
        L.emu_constraint_seq.argtypes = [C.c_void_p, dp, u8, C.c_int, u8, C.c_char_p, C.c_int, dp, dp, dp, dp]
        _lib = L
    return _lib


class ConstraintDriver:
    LIN, LOG = 0, 1

    def __init__(self, pattern, par="~T2004~", max_span=50, max_iloop=30, min_bpp=1e-4, tau=0.1, flags=0):
        from oracle import pyoracle as po
        if par in ("~T2004~", "~A2007~"):
            par = po.energy_param_text(par)
        self.max_span = max_span
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

    def run(self, x, seq, qual, cons, form=0):
        """dict(lnZ, P[(L+1), (W+1)], unpaired[L], ctx[L, 7], form: the form that wrote them); RuntimeError for a refused string"""
        import ctypes as C
        x = np.ascontiguousarray(x, dtype=np.float64)
        seq = np.ascontiguousarray(seq, dtype=np.uint8)
        qual = np.ascontiguousarray(qual, dtype=np.uint8)
        L = len(seq)
        W = min(L, self.max_span)
        assert len(cons) == L
        lnZ = C.c_double()
        P, unp, prof = np.full((L + 1, W + 1), np.nan), np.full(L, np.nan), np.full((L, 7), np.nan)
        dp, u8 = C.POINTER(C.c_double), C.POINTER(C.c_uint8)
        rc = driver().emu_constraint_seq(self.h, x.ctypes.data_as(dp), seq.ctypes.data_as(u8), L, qual.ctypes.data_as(u8), cons.encode(),
                                         form, C.byref(lnZ), P.ctypes.data_as(dp), unp.ctypes.data_as(dp), prof.ctypes.data_as(dp))
        if rc < 0:
            raise RuntimeError(driver().emu_last_error().decode())
        return dict(lnZ=lnZ.value, P=P, unpaired=unp, ctx=prof, form=rc)


class FixedOracle:
    """an oracle made with DBG_FIX_RSS, seen through the calls the table references make, for ONE structure: train_seq hands the
    structure on, bpp gives the pairs of the structure as the kept cells"""

    def __init__(self, o, db, W):
        self._o, self._db, self._W = o, db, W

    def __getattr__(self, name):
        return getattr(self._o, name)

    def train_seq(self, seq, qual, fix_rss=None, tables=False):
        return self._o.train_seq(seq, qual, fix_rss=self._db, tables=tables)

    def bpp(self, seq):
        L = len(seq)
        W = min(L, self._W)
        kept = np.zeros((L + 1, W + 1), dtype=np.uint8)
        for a, b in forced_pairs(self._db):
            kept[a, b - a + 1] = 1
        return None, kept, None, None
