"""Shared checks of the motif-conditional pair posteriors: two references built from the oracle alone --
enumerated_worlds (every structure over the kept cells, weighted once with every position on node 0 = the world without the
motif, and once with the rest = the world with it) and table_worlds (the oracle's pair posteriors of the mixture, those of an
oracle whose pattern rows of theta are -inf = the world without the motif, and the world with the motif solved from the mixture
identity) -- the test-only CPU driver of the product rule (tests/cond_emul.cpp), and the comparison of a record of
Engine.conditional_pairs (or of the driver) with either reference."""
import ctypes as C
import os
import subprocess

import numpy as np

from oracle import pyoracle as po
from tests import ctx_check as cc
from tests.emul import build as _emul_build
from tests.mea_mirror import mea_fold, pair_matrix
from tests.pair_check import oracle_pairs, unpaired_of

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cond_emul.cpp")
LIB = os.path.join(HERE, "libelemdp_cond_emul.so")
E_MIN = 1e-3          # P_motif solved from the mixture is compared only where exist_prob >= E_MIN: its error grows as 1 / e
_lib = None


# ---- reference 1: enumeration ---------------------------------------------------------------------------------------------------------

def enumerated_worlds(o, seq, qual):
    """dict(Pm, Pn: (L+1, W+1) arrays, e, shift, Zo, Zari, Znasi) by brute force; an empty world has P = 0 and shift NaN"""
    L = len(seq)
    t = o.train_seq(seq, qual)
    Zo, Za, Zn = t["Zo"], t["Zari"], t["Znasi"]
    _, kept, _, _ = o.bpp(seq)
    W = kept.shape[1] - 1
    Pm, Pn = np.zeros((L + 1, W + 1)), np.zeros((L + 1, W + 1))
    zeros = np.zeros(L, dtype=np.uint8)
    if np.isfinite(Zo):
        assert o.derivation_logz(seq, qual, None, zeros) == Zn
        dbs = cc.structures(kept, L, W)
        assert len(dbs) <= cc.MAX_STRUCTURES, len(dbs)
        tot_m = tot_n = 0.0
        for db in dbs:
            a, b = o.derivation_logz(seq, qual, db, None), o.derivation_logz(seq, qual, db, zeros)
            wn = np.exp(b - Zn) if np.isfinite(Zn) else 0.0
            wm = (np.exp(a - Za) - np.exp(b - Za)) if np.isfinite(Za) else 0.0
            tot_m += wm
            tot_n += wn
            stack = []
            for p, c in enumerate(db):
                if c == "(":
                    stack.append(p)
                elif c == ")":
                    i = stack.pop()
                    Pm[i, p + 1 - i] += wm
                    Pn[i, p + 1 - i] += wn
        assert not np.isfinite(Zn) or abs(tot_n - 1.0) <= 1e-12, tot_n
        assert not np.isfinite(Za) or abs(tot_m - 1.0) <= 1e-10, tot_m
    return finish_ref(Pm, Pn, kept, Zo, Za, Zn)


def finish_ref(Pm, Pn, kept, Zo, Za, Zn):
    both = np.isfinite(Za) and np.isfinite(Zn)
    e = 0.0 if not np.isfinite(Za) else 1.0 if not np.isfinite(Zn) else float(np.exp(Za - Zo))
    shift = float(np.abs(Pm - Pn)[kept.astype(bool)].sum()) if (both and Pm is not None) else np.nan
    return dict(Pm=Pm, Pn=Pn, e=e, shift=shift, Zo=Zo, Zari=Za, Znasi=Zn, kept=kept.astype(bool))


# ---- reference 2: the oracle's tables --------------------------------------------------------------------------------------------------

def none_params(x, hmm, softmax=False):
    """the parameters of the world without the motif: every row of theta but row 0 (the background) at -inf; a softmax model is
    handed over as its log-probabilities (the oracle for it is made without the softmax flag)"""
    xx = np.array(x, dtype=np.float64)
    off = 0
    for r, size in enumerate(hmm["theta_sizes"]):
        if softmax:
            xx[off:off + size] -= np.logaddexp.reduce(xx[off:off + size])
        if r > 0:
            xx[off:off + size] = -np.inf
        off += size
    return xx


def table_worlds(o, o_none, seq, qual):
    """dict as enumerated_worlds from pair_check.oracle_pairs of the mixture (o) and of the world without the motif (o_none: the same
    model with none_params); Pm is None where e < E_MIN (not comparable by this route), P the mixture's posteriors"""
    L = len(seq)
    t = o.train_seq(seq, qual)
    Zo, Za, Zn = t["Zo"], t["Zari"], t["Znasi"]
    if o.flags & po.NO_RSS:          # (a model without secondary structure keeps no pair)
        W = min(L, o._max_span())
        kept = np.zeros((L + 1, W + 1), dtype=np.uint8)
        P = Pn = np.zeros((L + 1, W + 1))
    else:
        _, kept, _, _ = o.bpp(seq)
        W = kept.shape[1] - 1
        P = oracle_pairs(o, seq, qual) if np.isfinite(Zo) else None
        Pn = oracle_pairs(o_none, seq, qual) if np.isfinite(Zn) else None
        if np.isfinite(Zn):
            tn = o_none.train_seq(seq, qual)
            assert tn["Zo"] == Zn and not np.isfinite(tn["Zari"]), (tn["Zo"], Zn, tn["Zari"])
        P = np.zeros((L + 1, W + 1)) if P is None else P
        Pn = np.zeros((L + 1, W + 1)) if Pn is None else Pn
    e = float(np.exp(Za - Zo)) if np.isfinite(Za) else 0.0
    if not np.isfinite(Za):
        Pm = np.zeros((L + 1, W + 1))
    elif e >= E_MIN:
        Pm = (P - (1.0 - e) * Pn) / e
    else:
        Pm = None
    r = finish_ref(Pm, Pn, kept, Zo, Za, Zn)
    r["P"] = P
    if Pm is None:          # (the shift needs both worlds)
        r["shift"] = None
    return r


def world_oracles(make, x):
    """(the oracle of make() with the parameters x set, a second one with none_params(x)): the pair of table_worlds"""
    o = make()
    o.set_params(x)
    on = make()
    on.set_params(none_params(x, o.hmm()))
    return o, on


def model_oracles(path):
    """the pair of table_worlds for a model file; a softmax model's second oracle takes the log-probabilities as plain theta"""
    o, x = cc.ctx_oracle_from_model(path)
    md = po.read_model(path)
    if md["softmax"]:
        flags = (po.NO_RSS if md["no_rss"] else 0) | (po.NO_PRF if md["no_prf"] else 0) | (po.NO_ENE if md["no_ene"] else 0)
        on = po.make_oracle(md["pattern"], md["max_span"], md["max_iloop"], min_bpp=md["min_bpp"], tau=md["tau"], flags=flags,
                            par_text=po.energy_param_text(md["ene_param"]))
        on.max_iloop_ = md["max_iloop"]          # (as ctx_check.ctx_oracle_from_model: the table references of the loop products read it)
    else:
        on = cc.ctx_oracle_from_model(path)[0]
    on.set_params(none_params(x, o.hmm(), softmax=md["softmax"]))
    return o, on


# ---- a record against a reference -------------------------------------------------------------------------------------------------------

def dense(rec, L, W):
    """(Pm, Pn, listed) of a record of Engine.conditional_pairs(x, 0.0)"""
    Pm, listed = pair_matrix(L, W, rec["i"], rec["j"], rec["p_motif"])
    Pn, _ = pair_matrix(L, W, rec["i"], rec["j"], rec["p_none"])
    return Pm, Pn, listed


def check_record(rec, ref, L, W, what="", enumerated=False):
    """a record at min_prob 0 against a reference: the list is the kept cells (span >= 1) in (i, j) order; P_none at rtol 1e-8 /
    atol 1e-12; P_motif at the same against the enumeration, at atol 1e-10 against the combined tables (where the reference has
    it); both unpaired vectors at rtol 1e-8 / atol 1e-10; exist_prob at rtol 1e-10; shift at rtol 1e-8 (plus 1e-12 per kept cell); the conventions of an empty
    world exactly"""
    Pm, Pn, listed = dense(rec, L, W)
    ki, kd = np.nonzero(ref["kept"])
    sel = (kd >= 1) & (ki + kd <= L)
    assert list(zip(rec["i"], rec["j"] - rec["i"])) == list(zip(ki[sel], kd[sel])), what
    m_empty, n_empty = not np.isfinite(ref["Zari"]), not np.isfinite(ref["Znasi"])
    np.testing.assert_allclose(Pn, ref["Pn"], rtol=1e-8, atol=1e-12, err_msg="P_none %s" % (what,))
    if ref["Pm"] is not None:
        np.testing.assert_allclose(Pm, ref["Pm"], rtol=1e-8, atol=1e-12 if enumerated else 1e-10, err_msg="P_motif %s" % (what,))
        np.testing.assert_allclose(rec["unpaired_motif"], unpaired_of(ref["Pm"], L), rtol=1e-8, atol=1e-10, err_msg="unpaired_motif %s" % (what,))
    np.testing.assert_allclose(rec["unpaired_none"], unpaired_of(ref["Pn"], L), rtol=1e-8, atol=1e-10, err_msg="unpaired_none %s" % (what,))
    if m_empty:
        assert rec["exist_prob"] == 0.0 and np.all(Pm == 0.0) and np.all(rec["unpaired_motif"] == 1.0), what
    if n_empty:
        assert rec["exist_prob"] == (0.0 if m_empty else 1.0) and np.all(Pn == 0.0) and np.all(rec["unpaired_none"] == 1.0), what
    if m_empty or n_empty:
        assert np.isnan(rec["shift"]), (what, rec["shift"])
    else:
        np.testing.assert_allclose(rec["exist_prob"], np.exp(ref["Zari"] - ref["Zo"]), rtol=1e-10, atol=0, err_msg="exist_prob %s" % (what,))
        if ref["shift"] is not None:
            # (a sum of |differences| over the kept cells: where the two folds agree it is all cancellation, and no better known
            # than the P it is made of -- the absolute term is the tightest absolute tolerance of a P, 1e-12, per kept cell)
            np.testing.assert_allclose(rec["shift"], ref["shift"], rtol=1e-8, atol=1e-12 * max(1, int(ref["kept"].sum())),
                                       err_msg="shift %s" % (what,))
    # probabilities, up to the rounding of their sums (in log space a term is exp(a + b - ln Z): at |ln Z| of a few thousand the
    # rounding of the exponent alone is 1e-12 relative per term -- the project's tolerance of `unpaired`, 1e-10, bounds it)
    for w in ("motif", "none"):
        assert rec["p_" + w].min(initial=0.0) >= 0.0 and rec["p_" + w].max(initial=0.0) <= 1.0 + 1e-10, what


def check_mixture(rec, pair, L, W, what=""):
    """e P_motif + (1 - e) P_none = P of the engine's own pair_posteriors(x, 0.0) entry (i, j, p, unpaired), atol 1e-12, and the
    same for unpaired, atol 1e-10"""
    ii, jj, pp, unp = pair
    assert np.array_equal(ii, rec["i"]) and np.array_equal(jj, rec["j"]), what
    e = rec["exist_prob"]
    np.testing.assert_allclose(e * rec["p_motif"] + (1.0 - e) * rec["p_none"], pp, rtol=0, atol=1e-12, err_msg="mixture %s" % (what,))
    np.testing.assert_allclose(e * rec["unpaired_motif"] + (1.0 - e) * rec["unpaired_none"], unp, rtol=0, atol=1e-10,
                               err_msg="mixture of unpaired %s" % (what,))


def check_structures(rec, L, W, gamma, what=""):
    """both MEA structures bit for bit against the host mirror on the record's own P and unpaired of each world"""
    Pm, Pn, listed = dense(rec, L, W)
    assert rec["structure_motif"] == mea_fold(Pm, listed, rec["unpaired_motif"], gamma)[0], (what, "motif")
    assert rec["structure_none"] == mea_fold(Pn, listed, rec["unpaired_none"], gamma)[0], (what, "none")


def same_records(a, b, rtol=0.0, atol=0.0):
    assert len(a) == len(b)
    for k, (r, s) in enumerate(zip(a, b)):
        assert set(r) == set(s), k
        for key in r:
            if isinstance(r[key], str):
                assert r[key] == s[key], (k, key)
            else:
                np.testing.assert_allclose(r[key], s[key], rtol=rtol, atol=atol, equal_nan=True, err_msg=str((k, key)))


# ---- the CPU driver of the product rule ---------------------------------------------------------------------------------------------

def driver():
    global _lib
    if _lib is None:
        srcs = [SRC] + _emul_build.SRCS[1:]
        deps = [SRC] + _emul_build.DEPS + [os.path.join(_emul_build.CSRC, f) for f in ("cond_rules.h", "pair_rules.h")]
        if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in deps):
            subprocess.check_call(["g++", "-std=c++14", "-O2", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-o", LIB] + srcs)
        L = C.CDLL(LIB)
        dp, u8 = C.POINTER(C.c_double), C.POINTER(C.c_uint8)
        L.emu_create.restype = C.c_void_p
        L.emu_create.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int]
        L.emu_destroy.argtypes = [C.c_void_p]
        L.emu_last_error.restype = C.c_char_p
        L.emu_set_fast.argtypes = [C.c_void_p, C.c_int]
        L.emu_cond_seq.argtypes = [C.c_void_p, dp, u8, C.c_int, u8, C.c_int, dp, dp, dp, dp, dp]
        _lib = L
    return _lib


class CondDriver:
    LIN, LOG = 0, 1

    def __init__(self, pattern, par="~T2004~", max_span=50, max_iloop=30, min_bpp=1e-4, tau=0.1, flags=0):
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

    def record(self, x, seq, qual, kept, form=0):
        """(a record as Engine.conditional_pairs(x, 0.0) gives it, the form that wrote it); kept: the oracle's kept cells, which
        the record lists"""
        x = np.ascontiguousarray(x, dtype=np.float64)
        seq = np.ascontiguousarray(seq, dtype=np.uint8)
        qual = np.ascontiguousarray(qual, dtype=np.uint8)
        L = len(seq)
        W = min(L, self.max_span)
        Pm, Pn = np.full((L + 1, W + 1), np.nan), np.full((L + 1, W + 1), np.nan)
        um, un, out2 = np.full(max(L, 1), np.nan), np.full(max(L, 1), np.nan), np.full(2, np.nan)
        dp, u8 = C.POINTER(C.c_double), C.POINTER(C.c_uint8)
        rc = driver().emu_cond_seq(self.h, x.ctypes.data_as(dp), seq.ctypes.data_as(u8), L, qual.ctypes.data_as(u8), form,
                                   Pm.ctypes.data_as(dp), Pn.ctypes.data_as(dp), um.ctypes.data_as(dp), un.ctypes.data_as(dp),
                                   out2.ctypes.data_as(dp))
        if rc < 0:
            raise RuntimeError(driver().emu_last_error().decode())
        ki, kd = np.nonzero(kept)
        sel = (kd >= 1) & (ki + kd <= L)
        ii, dd = ki[sel].astype(np.int32), kd[sel].astype(np.int32)
        assert np.all(Pm[~np.asarray(kept, dtype=bool)] == 0.0) and np.all(Pn[~np.asarray(kept, dtype=bool)] == 0.0)
        return dict(i=ii, j=ii + dd, p_motif=Pm[ii, dd], p_none=Pn[ii, dd], unpaired_motif=um[:L], unpaired_none=un[:L],
                    exist_prob=float(out2[0]), shift=float(out2[1])), rc
