"""Shared checks of the sampler: the test-only CPU driver (tests/sample_emul.cpp), a Python mirror of the
generator, the validity of a sample, and the sample frequencies against the oracle's posteriors."""
import ctypes as C
import os
import subprocess

import numpy as np

from tests.emul import build as _emul_build
from tests.mea_mirror import pairs_of

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "sample_emul.cpp")
LIB = os.path.join(HERE, "libelemdp_sample_emul.so")
_lib = None


def driver():
    """the CPU driver's library (built on first use, like tests/emul)"""
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
        L.emu_sample_uniform.restype = C.c_double
        L.emu_sample_uniform.argtypes = [C.c_uint64] * 4
        L.emu_set_fast.argtypes = [C.c_void_p, C.c_int]
        L.emu_sample_seq_lin.argtypes = [C.c_void_p, dp, u8, C.c_int, u8, C.c_int, C.c_uint64, C.c_uint64, C.c_char_p, u8, dp]
        _lib = L
    return _lib


class Driver:
    def __init__(self, pattern, par="~T2004~", max_span=50, max_iloop=30, min_bpp=1e-4, tau=0.1):
        if par == "~T2004~":      # (the engine's name of the default parameter set; the driver reads the text)
            from oracle import pyoracle as po
            par = open(po.DEFAULT_PAR).read()
        self.h = driver().emu_create(pattern.encode(), par.encode(), max_span, max_iloop, min_bpp, tau, 0)
        if not self.h:
            raise RuntimeError(driver().emu_last_error().decode())

    def set_fast(self, on):
        """inside tables through the table-driven unary phases (lin_fast.h), as k4_in runs them where the lists fit"""
        driver().emu_set_fast(self.h, int(bool(on)))

    def __del__(self):
        try:
            driver().emu_destroy(self.h)
        except Exception:
            pass

    def sample(self, x, seq, qual, n_samples, seed, index):
        """(rss strings, node rows, logp, status) of one sequence, as Engine.sample_structures gives them"""
        x = np.ascontiguousarray(x, dtype=np.float64)
        seq = np.ascontiguousarray(seq, dtype=np.uint8)
        qual = np.ascontiguousarray(qual, dtype=np.uint8)
        L = len(seq)
        rss = C.create_string_buffer(max(L * n_samples, 1))
        node = np.zeros(max(L * n_samples, 1), dtype=np.uint8)
        logp = np.zeros(n_samples)
        st = driver().emu_sample_seq_lin(self.h, x.ctypes.data_as(C.POINTER(C.c_double)), seq.ctypes.data_as(C.POINTER(C.c_uint8)),
                                         L, qual.ctypes.data_as(C.POINTER(C.c_uint8)), n_samples, seed, index, rss,
                                         node.ctypes.data_as(C.POINTER(C.c_uint8)), logp.ctypes.data_as(C.POINTER(C.c_double)))
        if st < 0:
            raise RuntimeError(driver().emu_last_error().decode())
        raw = rss.raw.decode("ascii")
        return [raw[t * L:(t + 1) * L] for t in range(n_samples)], node[:L * n_samples].reshape(n_samples, L), logp, st


M64 = (1 << 64) - 1


def mix(x):
    z = (x + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def uniform(seed, index, sample, draw):
    """the generator of sample_rules.h"""
    return (mix(mix(mix(mix(seed) ^ index) ^ sample) ^ draw) >> 11) * 2.0 ** -53


def motif_span(nodes, M):
    inside = np.nonzero((nodes != 0) & (nodes != M - 1))[0]
    return (int(inside[0]), int(inside[-1]) + 1) if len(inside) else (-1, -1)


def bound(p, n):
    return 5.0 * np.sqrt(np.maximum(p * (1.0 - p), 0.0) / n) + 2e-3


def check_distribution(rss, nodes, P, scan, M, what=""):
    """the samples' pair and unpaired frequencies against the oracle's posteriors P[i, d], the frequency of every motif start
    against exp(start), and the fraction with a motif against exist_prob"""
    N, L = nodes.shape
    f = np.zeros_like(P)
    starts = np.zeros(L)
    with_motif = 0
    for r, h in zip(rss, nodes):
        for i, d in pairs_of("".join("(" if c == "L" else ")" if c == "R" else "." for c in r)):
            f[i, d] += 1
        a, _ = motif_span(h, M)
        if a >= 0:
            starts[a] += 1
            with_motif += 1
    f /= N
    bad = np.abs(f - P) > bound(P, N)
    assert not bad.any(), (what, "pairs", [(int(i), int(d), f[i, d], P[i, d]) for i, d in zip(*np.nonzero(bad))][:5])
    unp_f = np.array([sum(r[p] not in "LR" for r in rss) for p in range(L)]) / N
    from tests.pair_check import unpaired_of
    unp_p = np.clip(unpaired_of(P, L), 0.0, 1.0)
    bad = np.abs(unp_f - unp_p) > bound(unp_p, N)
    assert not bad.any(), (what, "unpaired", np.nonzero(bad)[0][:5])
    ps = np.exp(scan["start"])
    bad = np.abs(starts / N - ps) > bound(ps, N)
    assert not bad.any(), (what, "start", [(int(p), starts[p] / N, ps[p]) for p in np.nonzero(bad)[0][:5]])
    pe = scan["exist_prob"]
    assert abs(with_motif / N - pe) <= bound(pe, N), (what, "exist", with_motif / N, pe)


def check_valid(rss, nodes, kept, W, M, node_names, what=""):
    """every sample a well-formed derivation: balanced dot-bracket of kept pairs of span <= W, rss letters that agree with it,
    O exactly on the exterior unpaired bases, the motif one run of the pattern's nodes in order, from the first to the last, whose
    bracket nodes sit on paired bases"""
    for t, (r, h) in enumerate(zip(rss, nodes)):
        L = len(r)
        assert len(r) == L and " " not in r, (what, t)
        db = "".join("(" if c == "L" else ")" if c == "R" else "." for c in r)
        prs = pairs_of(db)     # (raises on unbalanced brackets)
        depth = np.zeros(L, dtype=int)
        for i, d in prs:
            assert 2 <= d <= W and kept[i, d], (what, t, i, d)
            depth[i + 1:i + d - 1] += 1
        for p, c in enumerate(r):
            if c not in "LR":
                assert (c == "O") == (depth[p] == 0), (what, t, p, r)
        a, b = motif_span(h, M)
        if a >= 0:
            seg = h[a:b]
            assert np.all((seg != 0) & (seg != M - 1)), (what, t, "motif region is not contiguous")
            assert np.all(np.diff(seg.astype(int)) >= 0), (what, t, "motif nodes out of the pattern's order", list(seg))
            assert seg[0] == 1 and seg[-1] == M - 2, (what, t, "motif not whole")
            for p in range(a, b):
                if node_names[h[p]] in "()":
                    assert r[p] in "LR", (what, t, p)
        else:
            assert np.all((h == 0) | (h == M - 1)), (what, t)
