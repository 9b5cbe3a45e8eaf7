"""Maximum expected accuracy motif alignments and site lists on the GPU: Engine.mea_alignments against the
enumeration on the tiny and the multi-site cases of tests/test_node_mea_cpu.py, through the tie-robust checker against the
definitions over the oracle's tables at the shapes of tests/test_node_gpu.py, with both forms of the node pass in one call, across
groupings and a streamed batch, and through `scan --out-sites`.  k_node_mea takes one wave per sequence and walks the positions
one by one: it tiles neither positions nor sequences, so the lengths 1 .. 200 and batches of 8 to 17 sequences hold every shape
it has.  Its lanes take the nodes in rounds of 64; no pattern the engine accepts (at most 128 interval states) has more than 64
nodes, so a second round cannot be reached."""
import ctypes as C
import re

import numpy as np
import pytest

from rnaelem_amd import api, cli, io
from tests import ctx_check as cc
from tests import node_check as nc
from tests import node_mea_check as mc
from tests.test_ctx_gpu import pool_map, shape_batch
from tests.test_node_cpu import CASES, node_params, tiny_inputs
from tests.test_node_gpu import SHAPE_LENS, oracle_with, table_refs
from tests.test_node_mea_cpu import GAMMAS, HEADER, MARGIN, MULTI, MULTI_K, multi_reference
from tests.test_pair_shapes_gpu import P1, P2, PAR, batch
from tests.util import gpath

pytestmark = pytest.mark.gpu


def mea_call(eng, x, gamma, K, profile=False):
    """elemdp_node_mea with every output: per sequence the dict Engine.mea_alignments gives, plus the raw K slots as `slots`"""
    x = np.ascontiguousarray(x, dtype=np.float64)
    off, M, n = eng._off, eng.n_node, eng.n_seq
    n_pos = int(off[-1])
    prof = np.full(max(M * n_pos, 1), np.nan) if profile else None
    node = np.full(max(K * n_pos, 1), 255, dtype=np.uint8)
    ns = np.full(n, -7, dtype=np.int32)
    s0, s1 = np.full(n * K, -7, dtype=np.int32), np.full(n * K, -7, dtype=np.int32)
    sc, cf = np.zeros(n * K), np.zeros(n * K)
    dp, u8, i32 = C.POINTER(C.c_double), C.POINTER(C.c_uint8), C.POINTER(C.c_int32)
    eng._check(eng._lib.elemdp_node_mea(eng._h, x.ctypes.data_as(dp), eng.n_param, float(gamma), K,
                                        None if prof is None else prof.ctypes.data_as(dp), node.ctypes.data_as(u8),
                                        ns.ctypes.data_as(i32), s0.ctypes.data_as(i32), s1.ctypes.data_as(i32), sc.ctypes.data_as(dp),
                                        cf.ctypes.data_as(dp)))
    out = []
    for k in range(n):
        a, b, m = int(off[k]), int(off[k + 1]), int(ns[k])
        L = b - a
        assert 0 <= m <= K
        rows = node[K * a:K * b].reshape(K, L)
        sl = slice(k * K, (k + 1) * K)
        rec = dict(rows=rows[:m].copy(), start=s0[sl][:m].copy(), end=s1[sl][:m].copy(), score=sc[sl][:m].copy(),
                   confidence=cf[sl][:m].copy(), slots=dict(rows=rows, start=s0[sl], end=s1[sl], score=sc[sl], confidence=cf[sl]))
        if profile:
            rec["profile"] = prof[M * a:M * b].reshape(L, M).copy()
        out.append(rec)
    return out


def check_batch(eng, x, refs, gamma, K, what=""):
    """every sequence through the checker: against the table reference, and against the call's own profile"""
    names = eng.describe()["node"]
    got = mea_call(eng, x, gamma, K, profile=True)
    for k, (g, ref) in enumerate(zip(got, refs)):
        L = g["profile"].shape[0]
        if ref is None:
            assert len(g["start"]) == 0, (what, k)
            ref = nc.no_parse_profile(L, eng.n_node)
        mc.check_result(g, ref, names, gamma, K, what=(what, k, L, gamma, K))
        mc.check_result(g, ref, names, gamma, K, own_prof=g["profile"], what=(what, k, L, gamma, K, "own"))
        sites = sorted(zip(g["start"], g["end"]))
        assert all(a[1] <= b[0] for a, b in zip(sites, sites[1:])), (what, k, sites)
    return got


# ---- the tiny and the multi-site cases against the enumeration

@pytest.fixture(scope="module")
def tiny_brute():
    inputs = {case: tiny_inputs(case) for case in CASES}

    def one(_, case):
        pattern, L, flags, min_bpp = case
        x, s, q = inputs[case]
        o = nc.node_oracle(pattern, 50, 30, min_bpp=min_bpp, flags=flags)
        o.set_params(x)
        prof = nc.enumerated_profile(o, s, q)
        names = "".join(o.hmm()["node"])
        return {g: mc.brute_sites(prof, names, g, 1) for g in GAMMAS}

    return inputs, dict(zip(CASES, pool_map(lambda: None, one, CASES)))


@pytest.mark.parametrize("opts", [(), (("fast", 0),), (("pipeline", 3),)], ids=["default", "fast0", "pipeline3"])
def test_tiny_and_multi_site_cases_equal_the_enumeration(opts, tiny_brute):
    inputs, brute = tiny_brute
    for case in CASES:
        pattern, L, flags, min_bpp = case
        x, s, q = inputs[case]
        eng = api.Engine(pattern, PAR, 50, 30, min_bpp, 0.1, flags, 0)
        for k, v in opts:
            eng.set_option(k, v)
        eng.load_batch([s], [q])
        for gamma in GAMMAS:
            assert all(b[3] >= MARGIN for b in brute[case][gamma])
            (g,) = eng.mea_alignments(x, gamma, 1)
            mc.assert_equals_brute(g, brute[case][gamma], what=(opts, case, gamma))
    for pattern, L, gamma, sites, count in MULTI:
        x, s, q, names, prof = multi_reference(pattern, L)
        want = mc.brute_sites(prof, names, gamma, MULTI_K)
        assert all(b[3] >= MARGIN for b in want)
        eng = api.Engine(pattern, PAR, 50, 30, 1e-4, 0.1, 0, 0)
        for k, v in opts:
            eng.set_option(k, v)
        eng.load_batch([s], [q])
        (g,) = eng.mea_alignments(x, gamma, MULTI_K)
        mc.assert_equals_brute(g, want, what=(opts, pattern))
        if sites is not None:
            assert list(zip(g["start"], g["end"]))[:len(sites)] == sites


# ---- shapes through the checker

PIPELINE3 = (("pipeline", 3),)
_REFS = {}


def cached(key, compute):
    """the references of a case, computed once for the scaled-linear and the log-space form (the oracle is the slow part)"""
    if key not in _REFS:
        _REFS[key] = compute()
    return _REFS[key]


def engine_with(pattern, W, opts=()):
    eng = api.Engine(pattern, PAR, W, 30, 1e-4, 0.1, 0, 0)
    for k, v in opts:
        eng.set_option(k, v)
    return eng


def shape_case(pattern, W, lens):
    """(seqs, quals, x, the table references of the node profile) of a shape case"""
    def compute():
        seqs, quals = shape_batch(lens, seed=1000 * W + len(pattern) + len(lens), with_edge=(lens is SHAPE_LENS))
        x = node_params(engine_with(pattern, W))
        return seqs, quals, x, table_refs(oracle_with(pattern, x, W), seqs, quals, x)
    return cached(("shape", pattern, W, lens), compute)


W20_LENS, W70_LENS, LONG_LENS = (5, 19, 20, 21, 47), (66, 70, 93), (257, 300)


@pytest.mark.parametrize("pattern,W,lens", [(P1, 50, SHAPE_LENS), (P2, 50, SHAPE_LENS), (P1, 70, W70_LENS), (P1, 20, W20_LENS),
                                            (P1, 20, LONG_LENS)], ids=["P1-W50", "P2-W50", "P1-W70", "P1-W20", "P1-W20-long"])
def test_shapes_through_the_checker(pattern, W, lens):
    seqs, quals, x, refs = shape_case(pattern, W, lens)
    eng = engine_with(pattern, W)
    eng.load_batch(seqs, quals)
    found = 0
    first = {}
    for K in (1, 4):
        for gamma in GAMMAS:
            got = check_batch(eng, x, refs, gamma, K, what=(pattern, W))
            found += sum(len(g["start"]) for g in got)
            first[(K, gamma)] = [(g["slots"]["rows"][0], g["profile"]) for g in got]
    # K = 1 is slot 0 of K = 4.  (Two calls: the sum passes use LDS atomics and their profiles may differ in the last bits, so where
    # the rows differ they must tie under the profile of either call.)
    for gamma in GAMMAS:
        for (r1, _), (r4, p4) in zip(first[(1, gamma)], first[(4, gamma)]):
            if not np.array_equal(r1, r4):
                s1, s4 = mc.row_score(p4, r1, gamma), mc.row_score(p4, r4, gamma)
                assert abs(s1 - s4) <= 1e-12 * max(abs(s4), 1.0), (gamma, r1, r4)
    if pattern == P1:
        assert found > 0


@pytest.mark.parametrize("W,lens", [(20, W20_LENS), (70, W70_LENS), (20, LONG_LENS)], ids=["P1-W20", "P1-W70", "P1-W20-long"])
def test_shapes_in_the_log_space_form(W, lens):
    """pipeline 3: the node pass runs in k_dp<DP_SCAN> (NodeLog) and k_node_mea reads its profile by launch position; the
    references of the scaled-linear cases through the same checker, at every gamma for one site and for four"""
    seqs, quals, x, refs = shape_case(P1, W, lens)
    eng = engine_with(P1, W, PIPELINE3)
    eng.load_batch(seqs, quals)
    found = 0
    for K in (1, 4):
        for gamma in GAMMAS:
            found += sum(len(g["start"]) for g in check_batch(eng, x, refs, gamma, K, what=(W, "pipeline 3")))
    assert found > 0
    assert eng.last_timing()[2] == 0


MODELS = ["syn_sm.model", "syn_a2007.model", "2.model"]


def model_case(model):
    def compute():
        m = io.read_model(gpath(model))
        seqs, quals = batch((3, 13, 40, 97, 131), seed=len(model))
        make = lambda: nc.node_oracle_from_model(gpath(model))[0]
        return m, seqs, quals, table_refs(make, seqs, quals, m["x"], tau=m["tau"])
    return cached(("model", model), compute)


def check_model(model, opts):
    m, seqs, quals, refs = model_case(model)
    eng = io.engine_from_model(m)
    for k, v in opts:
        eng.set_option(k, v)
    eng.load_batch(seqs, quals)
    for K in (1, 4):
        for gamma in GAMMAS:
            check_batch(eng, m["x"], refs, gamma, K, what=(model, opts))
    return eng


@pytest.mark.parametrize("model", MODELS)
def test_models_through_the_checker(model):
    check_model(model, ())


@pytest.mark.parametrize("model", MODELS)
def test_models_in_the_log_space_form(model):
    """pipeline 3 (2.model: the no_rss branches of k_dp)"""
    eng = check_model(model, PIPELINE3)
    assert eng.last_timing()[2] == 0


def test_both_forms_of_the_node_pass_in_one_call():
    recs = io.read_fastq(gpath("syn_L150_n8.fq"))
    short_s, short_q = batch((4, 9, 16, 24), seed=40, neg_every=0)
    seqs = short_s[:2] + [s for _, s, _ in recs][:4] + short_s[2:]
    quals = short_q[:2] + [q for _, _, q in recs][:4] + short_q[2:]
    eng = api.Engine(P1, PAR, 50, 30, 1e-4, 0.1, 0, 0)
    eng.set_option("group", 2)
    eng.load_batch(seqs, quals)
    x = eng.initial_params(40.0)
    refs = table_refs(oracle_with(P1, x), seqs, quals, x)
    check_batch(eng, x, refs, 4.0, 4, what="lambda 40")
    assert 3 <= eng.last_timing()[2] < len(seqs)
    assert eng.last_timing()[2] > 0


def test_a_sequence_without_any_parse_has_no_site():
    o = nc.node_oracle(P1)
    eng = api.Engine(P1, PAR, 50, 30, 1e-4, 0.1, 0, 0)
    x, seqs, quals = cc.no_parse_inputs(node_params(eng), o.hmm())
    eng.load_batch(seqs, quals)
    refs = table_refs(oracle_with(P1, x), seqs, quals, x)
    assert refs[0] is None and refs[1] is not None
    for K in (1, 4):
        got = check_batch(eng, x, refs, 4.0, K, what="no parse")
        assert len(got[0]["start"]) == 0 and not got[0]["slots"]["rows"].any()


# ---- groupings, streaming, the profile flag, and what the call leaves alone

@pytest.fixture(scope="module")
def grouped():
    lens = [int(v) for v in np.linspace(20, 200, 9)][::-1]
    lens[2], lens[6] = lens[6], lens[2]
    seqs, quals = batch(lens, seed=5)
    base = api.Engine(P1, PAR, 50, 30, 1e-4, 0.1, 0, 0)
    base.load_batch(seqs, quals)
    x = node_params(base)
    refs = table_refs(oracle_with(P1, x), seqs, quals, x)
    return seqs, quals, base, x, refs


@pytest.mark.parametrize("opts", [(("group", 1),), (("group", 3),), (("max_resident", 2),)], ids=["group1", "group3", "streamed"])
def test_groupings_and_a_streamed_batch(opts, grouped):
    seqs, quals, base, x, refs = grouped
    eng = api.Engine(P1, PAR, 50, 30, 1e-4, 0.1, 0, 0)
    for k, v in opts:
        eng.set_option(k, v)
    eng.load_batch(seqs, quals)
    got = check_batch(eng, x, refs, 4.0, 4, what=opts)
    want = check_batch(base, x, refs, 4.0, 4, what="default")
    assert [len(g["start"]) for g in got] == [len(w["start"]) for w in want]
    assert sum(len(g["start"]) for g in got) > 0


def test_a_workgroup_of_the_log_space_form_takes_several_sequences(grouped):
    """pipeline 3 with option slots 3: log_scan_args asks for min(slots, n_seq) table slots and launches as many workgroups, so
    n_blocks = 3 workgroups take the n_seq = 9 unsorted sequences of L 20 .. 200 of the grouping tests off the atomic counter.
    Through the checker against the table references, not against another grouping."""
    seqs, quals, base, x, refs = grouped
    eng = api.Engine(P1, PAR, 50, 30, 1e-4, 0.1, 0, 0)
    eng.set_option("pipeline", 3)
    eng.set_option("slots", 3)
    eng.load_batch(seqs, quals)
    got = check_batch(eng, x, refs, 4.0, 4, what="slots 3")
    assert sum(len(g["start"]) for g in got) > 0
    assert (eng.slot_status()["slots"], eng.n_seq) == (3, 9)
    assert eng.last_timing()[2] == 0


def test_the_profile_flag_and_the_python_call(grouped):
    seqs, quals, base, x, refs = grouped
    raw = mea_call(base, x, 4.0, 4, profile=False)
    with_prof = base.mea_alignments(x, 4.0, 4, profile=True)
    without = base.mea_alignments(x, 4.0, 4)
    want = base.node_profiles(x)
    for k, (r, a, b, w) in enumerate(zip(raw, with_prof, without, want)):
        assert "profile" not in b and a["rows"].shape == (len(a["start"]), len(seqs[k]))
        nc.assert_profile(a["profile"], w, what=k, cols=range(base.n_node))
        # (the sum passes use LDS atomics: two calls may differ in the last bits, so the rows go through the checker)
        for g in (a, b):
            mc.check_result(g, refs[k], base.describe()["node"], 4.0, 4, what=k)
        assert len(r["start"]) == len(b["start"]) == len(a["start"])


def test_what_the_call_leaves_alone(grouped):
    seqs, quals, base, x, refs = grouped
    eng = api.Engine(P1, PAR, 50, 30, 1e-4, 0.1, 0, 0)
    eng.load_batch(seqs, quals)
    eng.train_eval(x)
    eng.seq_counts()
    eng.mea_alignments(x, 4.0, 4)
    with pytest.raises(api.ElemdpError) as err:      # (as after any scan-family call)
        eng.seq_counts()
    assert err.value.code == -4
    before, en0 = eng.scan(x)
    first = eng.pair_posteriors(x, 0.0)
    eng.mea_alignments(x, 4.0, 4)
    again = eng._pair_lists(sum(len(r[0]) for r in first), np.concatenate([r[3] for r in first]))
    for a, b in zip(first, again):
        assert all(np.array_equal(u, v) for u, v in zip(a, b))
    after, en1 = eng.scan(x)
    for a, b in zip(before, after):
        assert a["rss"] == b["rss"] and np.array_equal(a["psihat"], b["psihat"]) and (a["Ys"], a["Ye"]) == (b["Ys"], b["Ye"])
        for key in ("start", "inner", "end"):
            # (log posteriors of two scans: the sum passes gather through LDS atomics, so the linear values agree to rounding,
            # which is an absolute error of their logarithms)
            np.testing.assert_allclose(b[key], a[key], rtol=1e-10, atol=1e-12)


def test_refusals():
    eng = api.Engine(P1, PAR, 50, 30, 1e-4, 0.1, 0, 0)
    x = node_params(eng)
    with pytest.raises(api.ElemdpError) as err:
        mea_call_unloaded(eng, x)
    assert err.value.code == -4      # ELEMDP_ESTATE
    seqs, quals = batch((20, 31), seed=1)
    eng.load_batch(seqs, quals)
    for gamma in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(api.ElemdpError) as err:
            eng.mea_alignments(x, gamma, 1)
        assert err.value.code == -1, gamma      # ELEMDP_EINVAL
    for K in (0, 65):
        with pytest.raises(api.ElemdpError) as err:
            eng.mea_alignments(x, 1.0, K)
        assert err.value.code == -1, K
    dp = C.POINTER(C.c_double)
    none = [None] * 7
    assert eng._lib.elemdp_node_mea(eng._h, x.ctypes.data_as(dp), eng.n_param + 1, 1.0, 1, *none) == -1
    assert eng._lib.elemdp_node_mea(eng._h, None, eng.n_param, 1.0, 1, *none) == -1
    assert eng._lib.elemdp_node_mea(eng._h, x.ctypes.data_as(dp), eng.n_param, 1.0, 1, *none) == 0      # (every output may be NULL)
    assert len(eng.mea_alignments(x, 1.0, 64)) == 2


def mea_call_unloaded(eng, x):
    dp = C.POINTER(C.c_double)
    eng._check(eng._lib.elemdp_node_mea(eng._h, x.ctypes.data_as(dp), eng.n_param, 1.0, 1, *([None] * 7)))


# ---- command line

def test_command_line_writes_the_site_file(tmp_path):
    fq, model = gpath("positive_head6.fq"), gpath("trna_a.model")
    a1, sf, nf, n0 = (str(tmp_path / n) for n in ("a.raw", "sites.txt", "nodes.txt", "nodes0.txt"))
    cli.main(["scan", "-f", fq, "-q", model, "--out1", a1, "--out-sites", sf, "--site-gamma", "4", "--max-sites", "3"])
    alone = open(sf).read()
    cli.main(["scan", "-f", fq, "-q", model, "--out1", a1, "--out-sites", sf, "--site-gamma", "4", "--max-sites", "3", "--out-nodes", nf])
    cli.main(["scan", "-f", fq, "-q", model, "--out1", a1, "--out-nodes", n0])
    recs = io.read_fastq(fq)
    m = io.read_model(model)
    eng = io.engine_from_model(m)
    eng.load_batch([s for _, s, _ in recs], [q for _, _, q in recs])
    want = eng.mea_alignments(m["x"], 4.0, 3)
    names = eng.describe()["node"]
    for text in (alone, open(sf).read()):
        (tmp_path / "t.txt").write_text(text)
        got = io.read_sites(str(tmp_path / "t.txt"))
        assert [g[0] for g in got] == [r[0] for r in recs]
        for (rid, g), w in zip(got, want):
            assert np.array_equal(g["start"], w["start"]) and np.array_equal(g["end"], w["end"]), rid
            assert g["rows"] == ["".join(names[v] for v in row) for row in w["rows"]], rid
            np.testing.assert_allclose(g["score"], w["score"], rtol=2e-6, err_msg=rid)
            np.testing.assert_allclose(g["confidence"], w["confidence"], rtol=2e-6, err_msg=rid)
    assert sum(len(w["start"]) for w in want) > 0
    both, plain = io.read_node_records(nf), io.read_node_records(n0)
    for (ra, na, pa, ca), (rb, nb, pb, cb) in zip(both, plain):
        assert (ra, na) == (rb, nb)
        np.testing.assert_allclose(pa, pb, rtol=2e-6, atol=1e-12)
        np.testing.assert_allclose(ca, cb, rtol=2e-6, atol=1e-12)


def test_node_mea_symbol_is_declared_and_exported():
    declared = set(re.findall(r"\b(elemdp_[a-z_0-9]+)\s*\(", open(HEADER).read()))
    assert "elemdp_node_mea" in declared and "elemdp_node_mea" in api.SYMBOLS
    assert hasattr(api.load_library(), "elemdp_node_mea")
