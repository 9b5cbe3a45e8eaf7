"""Posterior motif-node profiles on the GPU: Engine.node_profiles against brute-force enumeration with the
oracle on the tiny batch of tests/test_node_cpu.py, against the definitions over the oracle's tables and the oracle's scan
identities at the shapes where the kernel has code of its own, across groupings and streamed batches, against the engine's own
context profiles rule by rule, against the node frequencies of the sampler, and through `scan --out-nodes`."""
import numpy as np
import pytest

from rnaelem_amd import api, cli, io
from tests import ctx_check as cc
from tests import node_check as nc
from tests.pair_check import check_scan, oracle_refs
from tests.sample_check import bound
from tests.test_ctx_gpu import pool_map, shape_batch
from tests.test_node_cpu import CASES, node_params, tiny_inputs
from tests.test_pair_shapes_gpu import P1, P2, PAR, batch, oracle_maker
from tests.util import gpath

pytestmark = pytest.mark.gpu

SHAPE_LENS = (1, 2, 5, 49, 50, 51, 107, 131, 200)      # 1, 2, 5, W-1, W, W+1, 2W+7, 131, 200 at W = 50


def oracle_with(pattern, x, W=50, C=30):
    def make():
        o = nc.node_oracle(pattern, W, C)
        o.set_params(x)
        return o
    return make


def table_refs(make, seqs, quals, x, tau=0.1):
    order = sorted(range(len(seqs)), key=lambda k: -len(seqs[k]))
    got = pool_map(make, lambda o, k: nc.table_profile(o, seqs[k], quals[k], x, tau=tau), order)
    out = [None] * len(seqs)
    for k, v in zip(order, got):
        out[k] = v
    return out


def check_profiles(eng, x, seqs, quals, refs, make=None, what="", row_atol=1e-12):
    """every entry against the table reference; rows sum to 1 within row_atol; entries in [0, 1]; no parse: exactly node 0; with
    make, the oracle's scan identities on every sequence that has a parse"""
    prof = eng.node_profiles(x)
    M = eng.n_node
    assert len(prof) == len(seqs)
    for k, (g, ref) in enumerate(zip(prof, refs)):
        L = len(seqs[k])
        assert g.shape == (L, M), (what, k)
        if ref is None:
            assert np.array_equal(g, nc.no_parse_profile(L, M)), (what, k)
            continue
        nc.assert_profile(g, ref, what=(what, k, L), cols=range(M))
        np.testing.assert_allclose(g.sum(axis=1), 1.0, rtol=0, atol=row_atol, err_msg=str((what, k, "row sums")))
        assert g.min() >= 0.0 and g.max() <= 1.0, (what, k)
    if make is not None:
        live = [k for k, r in enumerate(refs) if r is not None]
        pool_map(make, lambda o, k: nc.assert_oracle_identities(o, seqs[k], quals[k], prof[k], what=(what, k)), live)
    return prof


# ---- the tiny batch against the enumeration

@pytest.fixture(scope="module")
def tiny_refs():
    inputs = {case: tiny_inputs(case) for case in CASES}

    def one(_, case):
        pattern, L, flags, min_bpp = case
        x, s, q = inputs[case]
        o = nc.node_oracle(pattern, 50, 30, min_bpp=min_bpp, flags=flags)
        o.set_params(x)
        return nc.enumerated_profile(o, s, q)

    return inputs, dict(zip(CASES, pool_map(lambda: None, one, CASES)))


@pytest.mark.parametrize("opts", [(), (("fast", 0),), (("pipeline", 3),)], ids=["default", "fast0", "pipeline3"])
def test_tiny_batch_equals_the_enumeration(opts, tiny_refs):
    inputs, enum = tiny_refs
    for case in CASES:
        pattern, L, flags, min_bpp = case
        x, s, q = inputs[case]
        eng = api.Engine(pattern, PAR, 50, 30, min_bpp, 0.1, flags, 0)
        for k, v in opts:
            eng.set_option(k, v)
        eng.load_batch([s], [q])
        (g,) = eng.node_profiles(x)
        assert enum[case] is not None
        nc.assert_profile(g, enum[case], what=(opts, case), cols=range(eng.n_node))
        np.testing.assert_allclose(g.sum(axis=1), 1.0, rtol=0, atol=1e-12)
        assert eng.last_timing()[2] == 0      # (no sequence handed on by the range check; pipeline 3 runs none)


# ---- shapes against the definitions over the oracle's tables and the oracle's scan

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
    """(seqs, quals, x, the oracle maker, table references) of a shape case"""
    def compute():
        seqs, quals = shape_batch(lens, seed=1000 * W + len(pattern) + len(lens), with_edge=(lens is SHAPE_LENS))
        x = node_params(engine_with(pattern, W))
        make = oracle_with(pattern, x, W)
        return seqs, quals, x, make, table_refs(make, seqs, quals, x)
    return cached(("shape", pattern, W, lens), compute)


W20_LENS, W70_LENS, LONG_LENS = (5, 19, 20, 21, 47), (66, 70, 93), (257, 300)


@pytest.mark.parametrize("pattern,W,lens", [(P1, 50, SHAPE_LENS), (P2, 50, SHAPE_LENS), (P1, 20, W20_LENS), (P1, 70, W70_LENS),
                                            (P1, 20, LONG_LENS)], ids=["P1-W50", "P2-W50", "P1-W20", "P1-W70", "P1-W20-long"])
def test_shapes_against_the_table_definitions(pattern, W, lens):
    """(W = 70: the lanes of k_node_pos take the spans d = 1 + lane, 65 + lane, .., so a position with cells of span above 64 sums
    a second round per lane before the wave reduction; the lengths 1 .. 200 leave the last workgroup of a sequence, four positions
    each, partly empty; L = 257 and 300 at W = 20: positions beyond 256)"""
    seqs, quals, x, make, refs = shape_case(pattern, W, lens)
    eng = engine_with(pattern, W)
    eng.load_batch(seqs, quals)
    prof = check_profiles(eng, x, seqs, quals, refs, make, what=(pattern, W))
    assert sum(r is not None for r in refs) >= len(lens)
    assert max(p[:, 1:-1].sum(axis=1).max() for p in prof) > 0.05


@pytest.mark.parametrize("W,lens", [(20, W20_LENS), (70, W70_LENS), (20, LONG_LENS)], ids=["P1-W20", "P1-W70", "P1-W20-long"])
def test_shapes_in_the_log_space_form(W, lens):
    """pipeline 3: k_dp<DP_SCAN> and NodeLog fill the planes the position stage reads, addressed by launch position; the
    references of the scaled-linear cases, rows within 1e-10 (test_sequences_out_of_the_double_range_take_the_log_space_form)"""
    seqs, quals, x, make, refs = shape_case(P1, W, lens)
    eng = engine_with(P1, W, PIPELINE3)
    eng.load_batch(seqs, quals)
    prof = check_profiles(eng, x, seqs, quals, refs, make, what=(W, "pipeline 3"), row_atol=1e-10)
    assert sum(r is not None for r in refs) >= len(lens)
    assert max(p[:, 1:-1].sum(axis=1).max() for p in prof) > 0.05
    assert eng.last_timing()[2] == 0


MODELS = ["syn_sm.model", "syn_a2007.model", "2.model"]


def model_case(model):
    def compute():
        m = io.read_model(gpath(model))
        seqs, quals = batch((3, 13, 40, 97, 131), seed=len(model))
        make = lambda: nc.node_oracle_from_model(gpath(model))[0]
        return m, seqs, quals, make, table_refs(make, seqs, quals, m["x"], tau=m["tau"])
    return cached(("model", model), compute)


@pytest.mark.parametrize("model", MODELS)
def test_models_against_the_table_definitions(model):
    """softmax theta, the ~A2007~ energy parameters, and a model without secondary structure (2.model: rule 8 alone)"""
    m, seqs, quals, make, refs = model_case(model)
    eng = io.engine_from_model(m)
    eng.load_batch(seqs, quals)
    check_profiles(eng, m["x"], seqs, quals, refs, make, what=model)


@pytest.mark.parametrize("model", MODELS)
def test_models_in_the_log_space_form(model):
    """pipeline 3 (2.model: the no_rss branches of k_dp, the node profile by rule 8 alone)"""
    m, seqs, quals, make, refs = model_case(model)
    eng = io.engine_from_model(m)
    eng.set_option("pipeline", 3)
    eng.load_batch(seqs, quals)
    check_profiles(eng, m["x"], seqs, quals, refs, make, what=(model, "pipeline 3"), row_atol=1e-10)
    assert eng.last_timing()[2] == 0


def test_sequences_out_of_the_double_range_take_the_log_space_form():
    """lambda = 40: the long sequences leave the double range of the scaled-linear tables and go through the fused scan kernel
    (option group 2), the short ones stay on the scaled-linear path: both forms in one call.  Rows sum to 1 within 1e-10 here: in
    log space a term is exp(a + b - ln Z) with |ln Z| of a few thousand, so the exponent alone rounds at eps |ln Z| ~ 1e-12."""
    recs = io.read_fastq(gpath("syn_L150_n8.fq"))
    short_s, short_q = batch((4, 9, 16, 24), seed=40, neg_every=0)
    seqs = short_s[:2] + [s for _, s, _ in recs][:4] + short_s[2:]
    quals = short_q[:2] + [q for _, _, q in recs][:4] + short_q[2:]
    eng = api.Engine(P1, PAR, 50, 30, 1e-4, 0.1, 0, 0)
    eng.set_option("group", 2)
    eng.load_batch(seqs, quals)
    x = eng.initial_params(40.0)
    refs = table_refs(oracle_with(P1, x), seqs, quals, x)
    check_profiles(eng, x, seqs, quals, refs, what="lambda 40", row_atol=1e-10)
    assert 3 <= eng.last_timing()[2] < len(seqs)


def test_a_sequence_without_any_parse_sits_on_node_0():
    o = nc.node_oracle(P1)
    eng = api.Engine(P1, PAR, 50, 30, 1e-4, 0.1, 0, 0)
    x, seqs, quals = cc.no_parse_inputs(node_params(eng), o.hmm())
    eng.load_batch(seqs, quals)
    refs = table_refs(oracle_with(P1, x), seqs, quals, x)
    assert refs[0] is None and refs[1] is not None
    prof = check_profiles(eng, x, seqs, quals, refs, what="no parse", row_atol=1e-10)
    assert np.array_equal(prof[0], nc.no_parse_profile(len(seqs[0]), eng.n_node))


# ---- groupings, and what a call leaves alone

def test_groupings_agree_and_nothing_else_changes():
    lens = [int(v) for v in np.linspace(20, 280, 11)][::-1]
    lens[2], lens[7] = lens[7], lens[2]
    seqs, quals = batch(lens, seed=5)
    base = api.Engine(P1, PAR, 50, 30, 1e-4, 0.1, 0, 0)
    base.load_batch(seqs, quals)
    x = node_params(base)
    first = base.pair_posteriors(x, 0.0)
    ctx = base.context_profiles(x)
    want = base.node_profiles(x)
    again = base._pair_lists(sum(len(r[0]) for r in first), np.concatenate([r[3] for r in first]))
    for a, b in zip(first, again):       # (the list of the last pair call is still the first call's)
        assert all(np.array_equal(u, v) for u, v in zip(a, b))
    for a, b in zip(ctx, base.context_profiles(x)):
        np.testing.assert_allclose(b, a, rtol=1e-10, atol=1e-14)
    refs = oracle_refs(oracle_maker(P1, 50, 30, x), seqs, quals)
    check_scan(base, x, seqs, refs)
    for opts in ((("group", 3),), (("group_streams", 1),), (("group_streams", 2),), (("max_resident", 4),)):
        eng = api.Engine(P1, PAR, 50, 30, 1e-4, 0.1, 0, 0)
        for k, v in opts:
            eng.set_option(k, v)
        eng.load_batch(seqs, quals)
        got = eng.node_profiles(x)
        for k, (g, w) in enumerate(zip(got, want)):
            assert g.shape == w.shape
            np.testing.assert_allclose(g, w, rtol=1e-10, atol=1e-14, err_msg=str((opts, k)))


def test_a_workgroup_of_the_log_space_form_takes_several_sequences():
    """pipeline 3 with option slots 3: log_scan_args asks for min(slots, n_seq) table slots and launches as many workgroups, so
    n_blocks = 3 workgroups take the n_seq = 11 unsorted sequences of L 20 .. 280 off the atomic counter.  Against the table
    references, not against another grouping."""
    lens = [int(v) for v in np.linspace(20, 280, 11)][::-1]
    lens[2], lens[7] = lens[7], lens[2]
    seqs, quals = batch(lens, seed=5)
    eng = engine_with(P1, 50, PIPELINE3 + (("slots", 3),))
    eng.load_batch(seqs, quals)
    x = node_params(eng)
    refs = table_refs(oracle_with(P1, x), seqs, quals, x)
    check_profiles(eng, x, seqs, quals, refs, what="slots 3", row_atol=1e-10)
    assert sum(r is not None for r in refs) >= 10
    assert (eng.slot_status()["slots"], eng.n_seq) == (3, 11)
    assert eng.last_timing()[2] == 0


# ---- the engine's own context profiles, rule by rule

@pytest.mark.parametrize("opts", [(), (("pipeline", 3),)], ids=["default", "pipeline3"])
def test_the_parts_of_the_profile_are_the_context_columns(opts):
    """max_iloop 30: the L <- L part is U = H + B + I, the left / right bases of rules 1a / 1b are L / R, the rule-8 part is O, and
    rules 3a and 5a together are M (option node_rules: the rules that take part)"""
    seqs, quals = batch((30, 77, 131), seed=12)
    eng = api.Engine(P1, PAR, 50, 30, 1e-4, 0.1, 0, 0)
    for k, v in opts:
        eng.set_option(k, v)
    eng.load_batch(seqs, quals)
    x = node_params(eng)
    ctx = eng.context_profiles(x)
    whole = eng.node_profiles(x)
    parts = {}
    for name, bits in (("U", 1), ("M", 2 | 4), ("L", 8), ("R", 32), ("O", 16)):
        eng.set_option("node_rules", bits)
        parts[name] = [p.sum(axis=1) for p in eng.node_profiles(x)]
    eng.set_option("node_rules", 63)
    for k, (c, w) in enumerate(zip(ctx, whole)):
        np.testing.assert_allclose(w.sum(axis=1), 1.0, rtol=0, atol=1e-12)
        np.testing.assert_allclose(parts["U"][k], c[:, 3] + c[:, 4] + c[:, 5], rtol=1e-8, atol=1e-10, err_msg="U %d" % k)
        np.testing.assert_allclose(parts["L"][k], c[:, 1], rtol=1e-8, atol=1e-10, err_msg="L %d" % k)
        np.testing.assert_allclose(parts["R"][k], c[:, 2], rtol=1e-8, atol=1e-10, err_msg="R %d" % k)
        np.testing.assert_allclose(parts["O"][k], c[:, 0], rtol=1e-8, atol=1e-10, err_msg="O %d" % k)
        np.testing.assert_allclose(parts["M"][k], c[:, 6], rtol=1e-8, atol=1e-10, err_msg="M %d" % k)
    assert max(c[:, 6].max() for c in ctx) > 1e-3 and max(c[:, 3].max() for c in ctx) > 0.05


# ---- the sampler beyond enumeration

def test_node_frequencies_of_the_sampler_lie_within_the_bound_of_the_profile():
    N = 4000
    seqs, quals = batch((40, 71, 100), seed=8, n_every=0)
    eng = api.Engine(P1, PAR, 50, 30, 1e-4, 0.1, 0, 0)
    eng.load_batch(seqs, quals)
    x = node_params(eng)
    prof = eng.node_profiles(x)
    smp = eng.sample_structures(x, N, seed=3)
    for k, ((_, node, _, st), g) in enumerate(zip(smp, prof)):
        assert st == eng.SAMPLED
        rows = np.asarray(node).reshape(N, len(seqs[k]))
        for m in range(eng.n_node):
            f = (rows == m).mean(axis=0)
            bad = np.abs(f - g[:, m]) > bound(g[:, m], N)
            assert not bad.any(), (k, m, [(int(p), f[p], g[p, m]) for p in np.nonzero(bad)[0][:5]])
    assert max(g[:, 1:-1].sum(axis=1).max() for g in prof) > 0.05


# ---- command line

def test_command_line_writes_the_node_file(tmp_path):
    fq, model = gpath("positive_head6.fq"), gpath("trna_a.model")
    a1, nf = str(tmp_path / "a.raw"), str(tmp_path / "nodes.txt")
    cli.main(["scan", "-f", fq, "-q", model, "--out1", a1, "--out-nodes", nf, "--out-context", str(tmp_path / "c.txt")])
    recs = io.read_fastq(fq)
    got = io.read_node_records(nf)
    assert [g[0] for g in got] == [r[0] for r in recs]
    assert len(io.read_context_records(str(tmp_path / "c.txt"))) == len(recs)
    m = io.read_model(model)
    eng = io.engine_from_model(m)
    eng.load_batch([s for _, s, _ in recs], [q for _, _, q in recs])
    want = eng.node_profiles(m["x"])
    res, _ = eng.scan(m["x"])
    names = eng.describe()["node"]
    for (rid, nm, g, conf), w, r in zip(got, want, res):
        assert nm == names
        printed = np.array([[float(io.fmt(v)) for v in row] for row in w])
        # (the printed 6 digits; the tables are summed with LDS atomics, so a run differs from another in the last bits)
        np.testing.assert_allclose(g, printed, rtol=2e-6, atol=1e-12, err_msg=rid)
        np.testing.assert_allclose(conf, api.alignment_confidence(w, r["psihat"]), rtol=2e-6, atol=1e-12, err_msg=rid)


def test_calls_without_a_batch_or_an_output_are_refused():
    import ctypes as C
    eng = api.Engine(P1, PAR, 50, 30, 1e-4, 0.1, 0, 0)
    lib = api.load_library()
    x = np.zeros(eng.n_param)
    out = np.zeros(eng.n_node)
    dp = C.POINTER(C.c_double)
    assert lib.elemdp_node_profile(eng._h, x.ctypes.data_as(dp), eng.n_param, out.ctypes.data_as(dp)) == -4      # ELEMDP_ESTATE
    seqs, quals = batch((20,), seed=1)
    eng.load_batch(seqs, quals)
    assert lib.elemdp_node_profile(eng._h, x.ctypes.data_as(dp), eng.n_param, None) == -1      # ELEMDP_EINVAL
