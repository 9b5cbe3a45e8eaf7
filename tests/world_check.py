"""Shared checks of the scan posteriors in one world, built from the oracle and the existing *_check modules
alone.  Four references:

1. the world without the motif: each product's tables reference on an oracle whose theta rows other than row 0 are -inf
   (cond_check.none_params); its Zo is the original Znasi to the bit;
2. the world with the motif: X_motif = (X - (1 - e) X_none) / e from reference 1 and the mixture's tables reference, e =
   exp(Zari - Zo), held at the product's absolute tolerance times (2 - e) / e where every sequence of the batch has e >= E_MIN;
3. the enumeration (tiny sequences): the per-world structure weights of cond_check over ctx_check.structures, accumulated onto each
   product's events, and the node rows of node_check.alignments for the node profile;
4. the sampler: logp against derivation_logz(db, nodes) - Z_w, and the draws of the CPU driver tests/world_sample_emul.cpp."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np

from tests import access_check as ac
from tests import cond_check as cd
from tests import ctx_check as cc
from tests import helix_check as hc
from tests import joint_check as jc
from tests import loop_check as lc
from tests import node_check as nc
from tests import sample_check as sc
from tests import stem_check as stc
from tests.emul import build as _emul_build
from tests.mea_mirror import pair_matrix
from tests.pair_check import oracle_pairs, unpaired_of

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "world_sample_emul.cpp")
LIB = os.path.join(HERE, "libelemdp_world_sample_emul.so")
E_MIN = cd.E_MIN
WORLDS = ("motif", "none")
U = 6                     # the widest window of the accessibility references
KMAX = hc.KMAX
RTOL = 1e-8               # the project's relative tolerance of a posterior
# the existing absolute tolerance of each product (pair_check / cond_check: 1e-12 for P; the `unpaired` tolerance 1e-10 elsewhere)
ATOL = dict(pairs=1e-12, unpaired=1e-10, context=1e-10, nodes=1e-10, access=1e-10, loops=1e-10, helices=1e-10, stems=1e-10, joint=1e-10)
NODE_ROWS_MAX = 7000      # node rows the enumeration walks per sequence (L = 12 under every pattern of the tiny cases, L = 15 under `(.*)`)
_lib = None


# ---- references 1 and 2: the tables ---------------------------------------------------------------------------------------------------

def _tables(o, seq, qual, x, products):
    """{product: dense array} of the oracle o with the parameters x, None for a sequence without a parse"""
    L = len(seq)
    out = {}
    for p in products:
        if p == "pairs":
            o.set_params(x)
            P = oracle_pairs(o, seq, qual)
            out["pairs"] = P
            out["unpaired"] = None if P is None else unpaired_of(P, L)
        elif p == "context":
            out[p] = cc.table_profile(o, seq, qual, x)
        elif p == "nodes":
            out[p] = nc.table_profile(o, seq, qual, x)
        elif p == "access":
            r = ac.table_access(o, seq, qual, x, U)
            out[p] = None if r is None else r[0]
        elif p == "loops":
            r = lc.table_loops(o, seq, qual, x)
            out[p] = None if r is None else r[0]
        elif p == "helices":
            out[p] = hc.table_helices(o, seq, qual, x, kmax=KMAX)
        elif p == "stems":
            out[p] = stc.table_stems(o, seq, qual, x)
        elif p == "joint":
            out[p] = jc.table_joint(o, seq, qual, x)
        else:
            raise KeyError(p)
    return out


def table_worlds(o, o_none, x, x_none, seq, qual, products):
    """dict(e, Zo, Zari, Znasi, mixed, none, motif: {product: array}) of one sequence.  none: reference 1 (None for an empty world);
    motif: reference 2, None where the world is empty or e < E_MIN (not comparable by this route)"""
    o.set_params(x)
    t = o.train_seq(seq, qual)
    Zo, Za, Zn = t["Zo"], t["Zari"], t["Znasi"]
    mixed = _tables(o, seq, qual, x, products) if np.isfinite(Zo) else None
    none = None
    if np.isfinite(Zn):
        o_none.set_params(x_none)
        tn = o_none.train_seq(seq, qual)
        assert tn["Zo"] == Zn and not np.isfinite(tn["Zari"]), (tn["Zo"], Zn, tn["Zari"])
        none = _tables(o_none, seq, qual, x_none, products)
    e = float(np.exp(Za - Zo)) if np.isfinite(Za) else 0.0
    motif = None
    if np.isfinite(Za) and e >= E_MIN:
        if none is None:
            motif = mixed
        else:
            motif = {p: (mixed[p] - (1.0 - e) * none[p]) / e for p in mixed}
    return dict(e=e, Zo=Zo, Zari=Za, Znasi=Zn, mixed=mixed, none=none, motif=motif)


def motif_atol(product, e):
    """the absolute tolerance of reference 2: the product's own times (2 - e) / e -- X and (1 - e) X_none each carry the product's
    error, and the difference is divided by e"""
    return ATOL[product] * (2.0 - e) / e


def assert_world(got, ref, world, products=None, what=""):
    """the dense products of one sequence in one world ({product: array}) against table_worlds' reference of that world"""
    want = ref[world]
    assert want is not None, (what, world, "no reference")
    for p in (products or want):
        if p not in got:
            continue
        a, b = np.asarray(got[p]), np.asarray(want[p])
        assert a.shape == b.shape, (what, world, p, a.shape, b.shape)
        if world == "none":
            np.testing.assert_allclose(a, b, rtol=RTOL, atol=ATOL[p], equal_nan=True, err_msg=str((what, world, p)))
        else:
            np.testing.assert_allclose(a, b, rtol=RTOL, atol=motif_atol(p, ref["e"]), equal_nan=True, err_msg=str((what, world, p)))


# ---- reference 3: the enumeration -----------------------------------------------------------------------------------------------------

def access_of(db, L):
    a = np.zeros((L, U))
    run = 0
    for p in range(L - 1, -1, -1):
        run = run + 1 if db[p] == "." else 0
        a[p, :min(run, U)] = 1.0
    return a


def enumerated_worlds(o, seq, qual):
    """dict(e, Zo, Zari, Znasi, motif, none: {pairs (L+1, W+1), unpaired (L,), context (L, 7), access (L, U), loops (L, L+1, 5),
    nodes (L, M) where the sequence has at most NODE_ROWS_MAX node rows}) by brute force (None for an empty world).  The structure events take the weights of cond_check.enumerated_worlds
    -- exp(b - Znasi) without the motif, (exp(a) - exp(b)) / exp(Zari) with it, a and b the derivation weights of the structure with
    any node row and with every position on node 0 --, the node profile the weights of the node rows of node_check.alignments (the
    row of zeros is the world without the motif).  The total weight of a world is 1 within 1e-12."""
    L = len(seq)
    t = o.train_seq(seq, qual)
    Zo, Za, Zn = t["Zo"], t["Zari"], t["Znasi"]
    _, kept, _, _ = o.bpp(seq)
    W = kept.shape[1] - 1
    names = o.hmm()["node"]
    M = len(names)
    zeros = np.zeros(L, dtype=np.uint8)
    tail = ac.nan_tail(L, U)
    live = dict(motif=np.isfinite(Za), none=np.isfinite(Zn))
    acc = {w: dict(pairs=np.zeros((L + 1, W + 1)), context=np.zeros((L, 7)), access=np.zeros((L, U)), loops=np.zeros((L, L + 1, 5)),
                   nodes=np.zeros((L, M))) for w in WORLDS}
    tot = dict(motif=0.0, none=0.0)
    if np.isfinite(Zo):
        assert o.derivation_logz(seq, qual, None, zeros) == Zn
        dbs = cc.structures(kept, L, W)
        assert len(dbs) <= cc.MAX_STRUCTURES, len(dbs)
        for db in dbs:
            a, b = o.derivation_logz(seq, qual, db, None), o.derivation_logz(seq, qual, db, zeros)
            wt = dict(none=np.exp(b - Zn) if live["none"] else 0.0, motif=(np.exp(a - Za) - np.exp(b - Za)) if live["motif"] else 0.0)
            letters = cc.classify(db)
            loops = lc.loops_of(db)
            window = access_of(db, L)
            for w in WORLDS:
                v = wt[w]
                if v == 0.0:
                    continue
                tot[w] += v
                for i, j, _ in _pairs_of(db):
                    acc[w]["pairs"][i, j - i] += v
                for p, c in enumerate(letters):
                    acc[w]["context"][p, cc.LETTERS.index(c)] += v
                acc[w]["access"] += v * window
                for ty, i, j, _, _ in loops:
                    acc[w]["loops"][i, j, ty - 1] += v
        tot_rows = dict(motif=0.0, none=0.0)
        rows = list(itertools.islice(nc.alignments(L, names), NODE_ROWS_MAX + 1))
        with_nodes = len(rows) <= NODE_ROWS_MAX      # (else too many node rows to enumerate: the world's reference has no "nodes")
        for h in rows if with_nodes else ():
            w = "none" if not h.any() else "motif"
            if not live[w]:
                continue
            v = np.exp(o.derivation_logz(seq, qual, None, h) - (Zn if w == "none" else Za))
            tot_rows[w] += v
            acc[w]["nodes"][np.arange(L), h] += v
        for w in WORLDS:
            if live[w]:
                assert abs(tot[w] - 1.0) <= 1e-12, (w, tot[w])
                assert not with_nodes or abs(tot_rows[w] - 1.0) <= 1e-12, (w, "node rows", tot_rows[w])
            if not with_nodes:
                del acc[w]["nodes"]
    out = dict(e=float(np.exp(Za - Zo)) if live["motif"] else 0.0, Zo=Zo, Zari=Za, Znasi=Zn, kept=kept.astype(bool))
    for w in WORLDS:
        if not live[w]:
            out[w] = None
            continue
        acc[w]["unpaired"] = unpaired_of(acc[w]["pairs"], L)
        acc[w]["access"][tail] = np.nan
        out[w] = acc[w]
    return out


def _pairs_of(db):
    stack, out = [], []
    for p, c in enumerate(db):
        if c == "(":
            stack.append(p)
        elif c == ")":
            i = stack.pop()
            out.append((i, p + 1, None))
    return out


ENUM_PRODUCTS = ("pairs", "unpaired", "context", "nodes", "access", "loops")


def assert_enumerated(got, ref, world, products=ENUM_PRODUCTS, what=""):
    """the dense products of one sequence in one world against the enumeration, at the product's own tolerance"""
    want = ref[world]
    assert want is not None, (what, world)
    for p in products:
        if p not in got or p not in want:
            continue
        np.testing.assert_allclose(got[p], want[p], rtol=RTOL, atol=ATOL[p], equal_nan=True, err_msg=str((what, world, p)))


# ---- the conventions of an empty world: what each call returns today for a sequence without a parse -------------------------------------

def empty_world(L, W, M, K=0):
    """{product: array} of a sequence whose world is empty"""
    return dict(pairs=np.zeros((L + 1, W + 1)), unpaired=np.ones(L), context=cc.exterior_only(L), nodes=nc.no_parse_profile(L, M),
                access=ac.all_ones(L, U), loops=np.zeros((L, L + 1, 5)), helices=np.zeros((L, L + 1, KMAX)),
                stems=np.zeros((L, L + 1, K)), joint=jc.no_parse_joint(L, M))


# ---- an engine's products as dense arrays -----------------------------------------------------------------------------------------------

ALL_PRODUCTS = ("pairs", "context", "nodes", "access", "loops", "helices", "stems", "joint")


def engine_products(eng, x, world, seqs, products=ALL_PRODUCTS):
    """per sequence {product: dense array} of the engine's calls in one world ("mixed", "motif", "none"), lists at min_prob 0 as dense
    planes; with "loops" also loop_counts, with "stems" stem_counts, with "joint" joint_counts"""
    n = len(seqs)
    out = [dict() for _ in range(n)]
    Ls = [len(s) for s in seqs]
    Ws = [min(L, eng.max_span) for L in Ls]
    if "pairs" in products:
        for k, (ii, jj, pp, unp) in enumerate(eng.pair_posteriors(x, 0.0, world=world)):
            out[k]["pairs"] = pair_matrix(Ls[k], Ws[k], ii, jj, pp)[0]
            out[k]["unpaired"] = unp
    if "context" in products:
        for k, p in enumerate(eng.context_profiles(x, world=world)):
            out[k]["context"] = p
    if "nodes" in products:
        for k, p in enumerate(eng.node_profiles(x, world=world)):
            out[k]["nodes"] = p
    if "access" in products:
        for k, p in enumerate(eng.accessibility(x, U, world=world)):
            out[k]["access"] = p
    if "loops" in products:
        closing, two, counts = eng.loop_posteriors(x, 0.0, world=world)
        for k in range(n):
            out[k]["loops"] = lc.dense_from_closing(Ls[k], closing[k])[0]
            out[k]["loop_counts"] = counts[k]
            out[k]["two"] = lc.two_dict(two[k])
    if "helices" in products:
        for k, lst in enumerate(eng.helix_posteriors(x, 0.0, 1, KMAX, world=world)):
            out[k]["helices"] = hc.dense_from_list(Ls[k], KMAX, lst)
    if "stems" in products:
        K = len(eng.stem_slots())
        counts, lists = eng.stem_profiles(x, 0.0, world=world)
        for k in range(n):
            out[k]["stems"] = stc.dense_from_list(Ls[k], K, lists[k])
            out[k]["stem_counts"] = counts[k]
    if "joint" in products:
        counts, profs = eng.joint_profiles(x, profile=True, world=world)
        for k in range(n):
            out[k]["joint"] = profs[k]
            out[k]["joint_counts"] = counts[k]
    return out


def by_slots(ref, slots):
    """a reference's dense stems (L, L + 1, M, M) on the product's slots"""
    if ref is None or "stems" not in ref:
        return ref
    r = dict(ref)
    r["stems"] = stc.by_slot(np.clip(ref["stems"], 0.0, None), slots) if ref["stems"].ndim == 4 else ref["stems"]
    return r


def assert_mixture(mixed, motif, none, e, what="", count_rtol=0.0):
    """e X_motif + (1 - e) X_none = X_mixed at atol 1e-12, entry by entry over every array the three dicts share (two-loop dicts as
    the union of their keys); rtol is 0 for everything unless count_rtol is given (the mixture-identity test proper gives none).
    count_rtol: a relative term for the *_counts entries alone -- a count is a sum of probabilities, each
    held to 1e-12, so where the probabilities themselves carry that error (the log-space form at |ln Z| of thousands: a term is
    exp(a + b - ln Z), whose exponent rounds at eps |ln Z|) the bound of the sum scales with the count"""
    for p in mixed:
        if p == "two":
            keys = sorted(set(mixed[p]) | set(motif[p]) | set(none[p]))
            a = np.array([e * motif[p].get(k, 0.0) + (1.0 - e) * none[p].get(k, 0.0) for k in keys])
            b = np.array([mixed[p].get(k, 0.0) for k in keys])
        else:
            a, b = e * np.asarray(motif[p]) + (1.0 - e) * np.asarray(none[p]), np.asarray(mixed[p])
        np.testing.assert_allclose(a, b, rtol=count_rtol if p.endswith("_counts") else 0, atol=1e-12, equal_nan=True, err_msg=str((what, p)))


# ---- reference 4: the sampler ---------------------------------------------------------------------------------------------------------------

def driver():
    """the CPU driver of the sampler in a world (built on first use, like tests/emul)"""
    global _lib
    if _lib is None:
        srcs = [SRC] + _emul_build.SRCS[1:]
        deps = [SRC] + _emul_build.DEPS + [os.path.join(_emul_build.CSRC, "sample_rules.h")]
        if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in deps):
            subprocess.check_call(["g++", "-std=c++14", "-O2", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-o", LIB] + srcs)
        L = C.CDLL(LIB)
        dp, u8 = C.POINTER(C.c_double), C.POINTER(C.c_uint8)
        L.emu_create.restype = C.c_void_p
        L.emu_create.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int]
        L.emu_destroy.argtypes = [C.c_void_p]
        L.emu_last_error.restype = C.c_char_p
        L.emu_set_fast.argtypes = [C.c_void_p, C.c_int]
        L.emu_world_sample_seq_lin.argtypes = [C.c_void_p, dp, u8, C.c_int, u8, C.c_int, C.c_uint64, C.c_uint64, C.c_char_p, u8, dp, C.c_int]
        _lib = L
    return _lib


class WorldDriver:
    def __init__(self, pattern, par="~T2004~", max_span=50, max_iloop=30, min_bpp=1e-4, tau=0.1, flags=0):
        if par in ("~T2004~", "~A2007~"):
            from oracle import pyoracle as po
            par = po.energy_param_text(par)
        self.h = driver().emu_create(pattern.encode(), par.encode(), max_span, max_iloop, min_bpp, tau, flags)
        if not self.h:
            raise RuntimeError(driver().emu_last_error().decode())

    def __del__(self):
        try:
            driver().emu_destroy(self.h)
        except Exception:
            pass

    def sample(self, x, seq, qual, n_samples, seed, index, world):
        """(rss strings, node rows, logp, status) of one sequence in world 0, 1 or 2, as Engine.sample_structures gives them"""
        x = np.ascontiguousarray(x, dtype=np.float64)
        seq = np.ascontiguousarray(seq, dtype=np.uint8)
        qual = np.ascontiguousarray(qual, dtype=np.uint8)
        L = len(seq)
        rss = C.create_string_buffer(max(L * n_samples, 1))
        node = np.zeros(max(L * n_samples, 1), dtype=np.uint8)
        logp = np.zeros(n_samples)
        dp, u8 = C.POINTER(C.c_double), C.POINTER(C.c_uint8)
        st = driver().emu_world_sample_seq_lin(self.h, x.ctypes.data_as(dp), seq.ctypes.data_as(u8), L, qual.ctypes.data_as(u8), n_samples,
                                               seed, index, rss, node.ctypes.data_as(u8), logp.ctypes.data_as(dp), world)
        if st < 0:
            raise RuntimeError(driver().emu_last_error().decode())
        raw = rss.raw.decode("ascii")
        return [raw[t * L:(t + 1) * L] for t in range(n_samples)], node[:L * n_samples].reshape(n_samples, L), logp, st


def check_samples(o, seq, qual, sample, world, M, what=""):
    """one sequence's (rss, nodes, logp, status) in a world against the oracle o (parameters set): status NO_PARSE exactly for an
    empty world; every logp = derivation_logz(db, nodes) - Z_w at the tolerance of the sampler tests (each distinct derivation
    once); node 0 everywhere without the motif, an inner node somewhere with it"""
    rss, nodes, logp, status = sample
    t = o.train_seq(seq, qual)
    Zw = t["Zari"] if world == "motif" else t["Znasi"]
    if not np.isfinite(Zw):
        assert status == 1 and np.all(np.isnan(logp)) and not nodes.any() and all(r.strip() == "" for r in rss), (what, status)
        return 0
    assert status == 0 and np.all(np.isfinite(logp)), (what, status)
    seen = {}
    for k in range(len(rss)):
        if world == "none":
            assert not nodes[k].any(), (what, k, nodes[k])
        else:
            assert ((nodes[k] != 0) & (nodes[k] != M - 1)).any(), (what, k, nodes[k])
        key = (rss[k], nodes[k].tobytes())
        if key not in seen:
            seen[key] = o.derivation_logz(seq, qual, sc.dot_bracket(rss[k]), nodes[k])
        zd = seen[key]
        assert np.isfinite(zd) and abs(logp[k] - (zd - Zw)) <= sc.logp_atol(Zw), (what, k, logp[k], zd - Zw)
    return len(seen)
