"""Shared checks of the sampler: the test-only CPU driver (tests/sample_emul.cpp), a Python mirror of the
generator, the validity of a sample, the sample frequencies against the oracle's posteriors, the exact log-probability of a
sample against the oracle's weight of that one derivation (Oracle.derivation_logz), and check_sample_path, the whole check of
one sample call of an engine."""
import ctypes as C
import os
import subprocess
import threading
from concurrent.futures import ThreadPoolExecutor

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
        L.emu_sample_seq_lin_cap.argtypes = L.emu_sample_seq_lin.argtypes + [C.c_int]
        _lib = L
    return _lib


class Driver:
    def __init__(self, pattern, par="~T2004~", max_span=50, max_iloop=30, min_bpp=1e-4, tau=0.1, flags=0):
        if par in ("~T2004~", "~A2007~"):      # (the engine's names of the built-in parameter sets; the driver reads the text)
            from oracle import pyoracle as po
            par = po.energy_param_text(par)
        self.h = driver().emu_create(pattern.encode(), par.encode(), max_span, max_iloop, min_bpp, tau, flags)
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

    def sample(self, x, seq, qual, n_samples, seed, index, cap=None):
        """(rss strings, node rows, logp, status) of one sequence, as Engine.sample_structures gives them; cap: walk stacks of
        cap frames in place of sample_stack_cap(L)"""
        x = np.ascontiguousarray(x, dtype=np.float64)
        seq = np.ascontiguousarray(seq, dtype=np.uint8)
        qual = np.ascontiguousarray(qual, dtype=np.uint8)
        L = len(seq)
        rss = C.create_string_buffer(max(L * n_samples, 1))
        node = np.zeros(max(L * n_samples, 1), dtype=np.uint8)
        logp = np.zeros(n_samples)
        st = driver().emu_sample_seq_lin_cap(self.h, x.ctypes.data_as(C.POINTER(C.c_double)), seq.ctypes.data_as(C.POINTER(C.c_uint8)),
                                             L, qual.ctypes.data_as(C.POINTER(C.c_uint8)), n_samples, seed, index, rss,
                                             node.ctypes.data_as(C.POINTER(C.c_uint8)), logp.ctypes.data_as(C.POINTER(C.c_double)),
                                             stack_cap(L) if cap is None else cap)
        if st < 0:
            raise RuntimeError(driver().emu_last_error().decode())
        raw = rss.raw.decode("ascii")
        return [raw[t * L:(t + 1) * L] for t in range(n_samples)], node[:L * n_samples].reshape(n_samples, L), logp, st


def stack_cap(L):
    """sample_stack_cap of sample_rules.h"""
    return L + 4


def driver_from_model(m):
    """the CPU driver of a model read by io.read_model (its flags have the oracle's and the driver's bit values)"""
    return Driver(m["pattern"], m["ene_param"], m["max_span"], m["max_iloop"], m["min_bpp"], m["tau"], m["flags"])


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


# ---- the exact log-probability of a sample ---------------------------------------------------------------------------------------

LOGZ_RTOL = 1e-10     # the project's tolerance of a log partition function (test_tables_of_single_sequences)


def logp_atol(Zo):
    """logp = derivation_logz - Zo: LOGZ_RTOL on both terms, each at most |Zo| in size (or 1)"""
    return 2 * LOGZ_RTOL * max(1.0, abs(Zo))


def dot_bracket(rss):
    return "".join("(" if c == "L" else ")" if c == "R" else "." for c in rss)


def oracle_map(make_oracle, fn, jobs):
    """[fn(o, job) for job in jobs] over pair_check.n_workers() threads, one oracle handle of make_oracle() per thread (the
    oracle's C calls release the GIL)"""
    from tests.pair_check import n_workers
    local = threading.local()

    def one(job):
        if not hasattr(local, "o"):
            local.o = make_oracle()
        return fn(local.o, job)

    with ThreadPoolExecutor(max_workers=n_workers()) as ex:
        return list(ex.map(one, jobs))


def oracle_zo(make_oracle, seqs, quals):
    """Zo = log Z(ari, nasi) per sequence (-inf: no parse), from one unconstrained inside pass"""
    order = sorted(range(len(seqs)), key=lambda k: -len(seqs[k]))
    z = oracle_map(make_oracle, lambda o, k: o.derivation_logz(seqs[k], quals[k], None, None), order)
    out = [None] * len(seqs)
    for k, v in zip(order, z):
        out[k] = v
    return out


def pick_samples(n_samples, n_check, rng):
    """sample indices to check: 0, 63, 64 and the last one where they exist (both lane rounds of k_sample and the seam between
    them), the rest drawn by rng, n_check in all (or every sample)"""
    must = sorted({t for t in (0, 63, 64, n_samples - 1) if 0 <= t < n_samples})
    rest = [t for t in range(n_samples) if t not in must]
    more = max(0, min(n_check - len(must), len(rest)))
    return sorted(must + [int(t) for t in rng.choice(rest, size=more, replace=False)]) if more else must


def check_exact_logp(make_oracle, seqs, quals, Zo, samples, picks, what=""):
    """logp == derivation_logz(rss, nodes) - Zo within logp_atol(Zo) for the samples picks[k] of every sequence k (samples[k] =
    (rss, nodes, logp, status); a derivation picked twice is computed once).  Returns the largest |logp - oracle| / max(1, |Zo|)."""
    jobs, seen = [], set()
    for k, ts in enumerate(picks):
        rss, nodes, logp, _ = samples[k]
        for t in ts:
            key = (k, rss[t], nodes[t].tobytes())
            if key not in seen:
                seen.add(key)
                jobs.append((k, t))
    jobs.sort(key=lambda kt: -len(seqs[kt[0]]))
    z = oracle_map(make_oracle, lambda o, kt: o.derivation_logz(seqs[kt[0]], quals[kt[0]], dot_bracket(samples[kt[0]][0][kt[1]]),
                                                               samples[kt[0]][1][kt[1]]), jobs)
    worst = 0.0
    for (k, t), zd in zip(jobs, z):
        lp = samples[k][2][t]
        err = abs(lp - (zd - Zo[k]))
        assert np.isfinite(zd) and err <= logp_atol(Zo[k]), (what, "logp", k, t, lp, zd - Zo[k], err, Zo[k])
        worst = max(worst, err / max(1.0, abs(Zo[k])))
    return worst


def distinct(rss, nodes):
    """{(rss, node bytes): [sample indices]} in order of first appearance"""
    out = {}
    for t, (r, h) in enumerate(zip(rss, nodes)):
        out.setdefault((r, h.tobytes()), []).append(t)
    return out


def check_sample_path(eng, seqs, quals, x, make_oracle, n_samples, seed, drv=None, index_base=0, mask_eng=None, refs=None,
                      n_check=16, log_all=False, count_flagged=True, dist="all", what=""):
    """The whole check of one sample call of an engine with the batch loaded.
    (a) status SAMPLED, or NO_PARSE exactly where the oracle's Zo is not finite; no NaN logp in a sampled sequence
    (b) check_valid on every sample (each distinct one once) on the kept cells of mask_eng (default: eng)
    (c) the CPU driver drv (the engine's model and x) draws the same samples with index index_base + k: at least 99.9 % of the
        case's samples identical in (rss, nodes).  Left out only for sequences in the log-space form, which the driver does
        not have: all of them with log_all (pipeline 3), else those whose scaled-linear Z leaves the double range in the driver
        as well (NO_PARSE or a NaN logp there although the oracle has a parse); with count_flagged their number must be the
        engine's own count, last_timing()[2]
    (d) logp == derivation_logz - Zo within logp_atol for n_check samples per sequence (4 for L > 1000), pick_samples
    (e) with refs (pair_check.oracle_refs): check_distribution of every sampled sequence (dist "log": of those in the log-space
        form only)
    Returns dict(res, Zo, same, total, share, worst, n_log)."""
    mask_eng = mask_eng or eng
    names = eng.describe()["node"]
    M = len(names)
    res = eng.sample_structures(x, n_samples, seed=seed, index_base=index_base)
    n_flagged = int(eng.last_timing()[2])
    assert len(res) == len(seqs)
    Zo = [r["scan"]["ZL"] for r in refs] if refs is not None else oracle_zo(make_oracle, seqs, quals)
    for k, (rss, nodes, logp, st) in enumerate(res):          # (a), (b)
        L = len(seqs[k])
        assert len(rss) == n_samples and nodes.shape == (n_samples, L) and len(logp) == n_samples, (what, k)
        if not np.isfinite(Zo[k]):
            assert st == eng.NO_PARSE, (what, "status", k, st)
            continue
        assert st == eng.SAMPLED, (what, "status", k, st, Zo[k])
        assert np.all(np.isfinite(logp)) and np.all(logp <= logp_atol(Zo[k])), (what, "logp", k)
        first = [ts[0] for ts in distinct(rss, nodes).values()]
        check_valid([rss[t] for t in first], nodes[first], mask_eng.pairs(k)[0], min(L, eng.max_span), M, names, what=(what, k))
    same = total = n_log = 0
    differ = [[] for _ in seqs]
    log_form = [log_all] * len(seqs)
    if not log_all:                                           # (c)
        assert drv is not None
        for k, (rss, nodes, logp, st) in enumerate(res):
            d_rss, d_nodes, d_logp, d_st = drv.sample(x, seqs[k], quals[k], n_samples, seed, index_base + k)
            if d_st != 0 or not np.all(np.isfinite(d_logp)):
                assert d_st in (0, 1), (what, "driver refused", k)
                n_log += 1                                    # (the scaled-linear tables left the double range, or no parse)
                log_form[k] = True
                continue
            assert st == eng.SAMPLED, (what, k)
            total += n_samples
            for t in range(n_samples):
                if rss[t] == d_rss[t] and np.array_equal(nodes[t], d_nodes[t]):
                    same += 1
                else:
                    differ[k].append(t)
        if count_flagged:
            assert n_log == n_flagged, (what, "sequences in the log-space form", n_log, n_flagged)
        assert same >= 0.999 * total, (what, "draws against the CPU driver", same, total)
    rng = np.random.default_rng(seed + 1000003 * n_samples)   # (d)
    picks = []
    for k, (rss, nodes, logp, st) in enumerate(res):
        if st != eng.SAMPLED:
            picks.append([])
            continue
        ts = pick_samples(n_samples, 4 if len(seqs[k]) > 1000 else n_check, rng)
        picks.append(sorted(set(ts) | set(differ[k])))        # (every sample that differs from the driver's has to be exact)
    worst = check_exact_logp(make_oracle, seqs, quals, Zo, res, picks, what=what)
    if refs is not None:                                      # (e)
        for k, ((rss, nodes, logp, st), ref) in enumerate(zip(res, refs)):
            if st == eng.SAMPLED and (dist == "all" or log_form[k]):
                check_distribution(rss, nodes, ref["P"], ref["scan"], M, what=(what, k))
    share = same / total if total else float("nan")
    print("sample case %s: %d sequences, driver share %s (%d of %d), log form %d, max |logp - oracle| / max(1, |Zo|) = %.3g"
          % (what, len(seqs), "%.5f" % share if total else "n/a", same, total, n_log, worst))
    return dict(res=res, Zo=Zo, same=same, total=total, share=share, worst=worst, n_log=n_log)
