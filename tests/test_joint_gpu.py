"""Joint node-by-context posteriors on the GPU: Engine.joint_profiles against the enumeration of structure x
node row with the oracle on the enumerated cases of tests/joint_check.py, against the definitions over the oracle's tables at the
shapes where the kernels have code of their own, against the CPU driver of the product rule at lengths that cross the tiles of
the per-sequence stages, against the engine's own node and context profiles, across groupings and streamed batches, and
through `scan --out-logo`."""
import ctypes as C

import numpy as np
import pytest

from rnaelem_amd import api, cli, io
from tests import ctx_check as cc
from tests import joint_check as jc
from tests.test_ctx_gpu import pool_map
from tests.test_pair_shapes_gpu import P1, P2, PAR, batch
from tests.util import gpath

pytestmark = pytest.mark.gpu


def oracle_with(pattern, x, W=50, C=30):
    def make():
        o = jc.joint_oracle(pattern, W, C)
        o.set_params(x)
        return o
    return make


def table_refs(make, seqs, quals, x, tau=0.1):
    order = sorted(range(len(seqs)), key=lambda k: -len(seqs[k]))
    got = pool_map(make, lambda o, k: jc.table_joint(o, seqs[k], quals[k], x, tau=tau), order)
    out = [None] * len(seqs)
    for k, v in zip(order, got):
        out[k] = v
    return out


def check_joint(eng, x, seqs, refs, what="", row_atol=1e-12):
    """every entry against the reference; sum_{m,c} J = 1 within row_atol; entries in [0, 1]; no parse: exactly (node 0, O); the
    counts against the sum of the profile over the positions; profile=False gives the same counts"""
    counts, prof = eng.joint_profiles(x, profile=True)
    M = eng.n_node
    assert counts.shape == (len(seqs), M, 7, 5) and len(prof) == len(seqs)
    for k, (g, ref) in enumerate(zip(prof, refs)):
        L = len(seqs[k])
        assert g.shape == (L, M, 7), (what, k)
        if ref is None:
            assert np.array_equal(g, jc.no_parse_joint(L, M)), (what, k)
        else:
            jc.assert_joint(g, ref, what=(what, k, L))
            np.testing.assert_allclose(g.sum(axis=(1, 2)), 1.0, rtol=0, atol=row_atol, err_msg=str((what, k, "row sums")))
            assert g.min() >= 0.0 and g.max() <= 1.0, (what, k)
        np.testing.assert_allclose(counts[k], jc.counts_of(g, seqs[k]), rtol=1e-13, atol=1e-13 * max(L, 1), err_msg=str((what, k, "counts")))
    return counts, prof


# ---- the enumerated cases

@pytest.mark.parametrize("opts", [(), (("fast", 0),), (("pipeline", 3),)], ids=["default", "fast0", "pipeline3"])
def test_enumerated_cases(opts):
    for case in jc.CASES:
        pattern, L, flags, min_bpp = case
        x, s, q, _, enum = jc.tiny_reference(case)
        eng = api.Engine(pattern, PAR, 50, 30, min_bpp, 0.1, flags, 0)
        for k, v in opts:
            eng.set_option(k, v)
        eng.load_batch([s], [q])
        assert enum is not None
        check_joint(eng, x, [s], [enum], what=(opts, case))
        assert eng.last_timing()[2] == 0      # (no sequence handed on by the range check; pipeline 3 runs none)


# ---- shapes against the definitions over the oracle's tables

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
    """(seqs, quals, x, table references) of a shape case"""
    def compute():
        seqs, quals = batch(lens, seed=1000 * W + len(pattern) + len(lens))
        x = jc.joint_params(engine_with(pattern, W))
        return seqs, quals, x, table_refs(oracle_with(pattern, x, W), seqs, quals, x)
    return cached(("shape", pattern, W, lens), compute)


def long_case():
    """L = 257 and 300 at W = 20, the references from the CPU driver of the product rule"""
    def compute():
        seqs, quals = batch((257, 300), seed=77, n_every=0)
        eng = engine_with(P1, 20)
        x = jc.joint_params(eng)
        drv = jc.JointDriver(P1, PAR, 20, 30, 1e-4, 0.1, 0, n_node=eng.n_node)
        return seqs, quals, x, [drv.joint(x, s, q, 0)[0] for s, q in zip(seqs, quals)]
    return cached("long", compute)


W20_LENS, W70_LENS = tuple(range(1, 61)), (107,)


@pytest.mark.parametrize("pattern,W,lens", [(P1, 20, W20_LENS), (P2, 20, W20_LENS), (P1, 70, W70_LENS)],
                         ids=["P1-W20", "P2-W20", "P1-W70"])
def test_shapes_against_the_table_definitions(pattern, W, lens):
    """(L = 1 .. 60: the last workgroup of a sequence, four rows or positions each, is partly empty, rows shorter and longer than
    W; W = 70: a position with cells of span above 64 sums a second round per lane before the wave reduction)"""
    seqs, quals, x, refs = shape_case(pattern, W, lens)
    eng = engine_with(pattern, W)
    eng.load_batch(seqs, quals)
    _, prof = check_joint(eng, x, seqs, refs, what=(pattern, W))
    assert sum(r is not None for r in refs) >= len(lens) - 1
    assert max(p[:, 1:-1, 3].sum(axis=1).max() for p in prof) > 0.05


@pytest.mark.parametrize("W,lens", [(20, W20_LENS), (70, W70_LENS)], ids=["P1-W20", "P1-W70"])
def test_shapes_in_the_log_space_form(W, lens):
    """pipeline 3: k_dp<DP_SCAN> and JointLog on the per-thread vectors of jnt.vec, the X scratch of the workgroup, the counts
    stage by launch position; the references of the scaled-linear cases, sums within 1e-10 (Rounding)"""
    seqs, quals, x, refs = shape_case(P1, W, lens)
    eng = engine_with(P1, W, PIPELINE3)
    eng.load_batch(seqs, quals)
    _, prof = check_joint(eng, x, seqs, refs, what=(W, "pipeline 3"), row_atol=1e-10)
    assert sum(r is not None for r in refs) >= len(lens) - 1
    assert max(p[:, 1:-1, 3].sum(axis=1).max() for p in prof) > 0.05
    assert eng.last_timing()[2] == 0


def test_long_sequences_against_the_cpu_driver():
    """L = 257 and 300 at W = 20 cross the tiles of 256 of the per-sequence stages"""
    seqs, quals, x, refs = long_case()
    eng = engine_with(P1, 20)
    eng.load_batch(seqs, quals)
    check_joint(eng, x, seqs, refs, what="long")


def test_long_sequences_in_the_log_space_form():
    """the same under pipeline 3"""
    seqs, quals, x, refs = long_case()
    eng = engine_with(P1, 20, PIPELINE3)
    eng.load_batch(seqs, quals)
    check_joint(eng, x, seqs, refs, what="long, pipeline 3", row_atol=1e-10)
    assert eng.last_timing()[2] == 0


# ---- the two marginal identities against the handle's own calls

@pytest.mark.parametrize("opts", [(), (("pipeline", 3),)], ids=["default", "pipeline3"])
def test_marginals_are_the_node_and_the_context_profiles_of_the_same_handle(opts):
    seqs, quals = batch((30, 77, 131), seed=12)
    eng = api.Engine(P1, PAR, 50, 30, 1e-4, 0.1, 0, 0)
    for k, v in opts:
        eng.set_option(k, v)
    eng.load_batch(seqs, quals)
    x = jc.joint_params(eng)
    node, ctx = eng.node_profiles(x), eng.context_profiles(x)
    _, prof = eng.joint_profiles(x, profile=True)
    tol = 1e-10 if opts else 1e-12        # (the log-space form: DESIGN.md section 15, Rounding)
    for k, g in enumerate(prof):
        np.testing.assert_allclose(g.sum(axis=2), node[k], rtol=0, atol=tol, err_msg="nodes %d" % k)
        np.testing.assert_allclose(g.sum(axis=1), ctx[k], rtol=0, atol=tol, err_msg="context %d" % k)
        np.testing.assert_allclose(g.sum(axis=(1, 2)), 1.0, rtol=0, atol=tol)
    assert max(g[:, 1:-1, 6].max() for g in prof) > 1e-4 and max(g[:, 1:-1, 3].max() for g in prof) > 0.05


MODELS = ["syn_sm.model", "syn_a2007.model", "2.model"]


def model_case(model):
    def compute():
        m = io.read_model(gpath(model))
        seqs, quals = batch((3, 13, 40, 97), seed=len(model))
        refs = table_refs(lambda: jc.joint_oracle_from_model(gpath(model))[0], seqs, quals, m["x"], tau=m["tau"])
        return m, seqs, quals, refs
    return cached(("model", model), compute)


@pytest.mark.parametrize("model", MODELS)
def test_models_against_the_table_definitions(model):
    """softmax theta, the ~A2007~ energy parameters, and a model without secondary structure (2.model: rule 8 alone)"""
    m, seqs, quals, refs = model_case(model)
    eng = io.engine_from_model(m)
    eng.load_batch(seqs, quals)
    check_joint(eng, m["x"], seqs, refs, what=model)


@pytest.mark.parametrize("model", MODELS)
def test_models_in_the_log_space_form(model):
    """pipeline 3 (2.model: the no_rss branches of k_dp)"""
    m, seqs, quals, refs = model_case(model)
    eng = io.engine_from_model(m)
    eng.set_option("pipeline", 3)
    eng.load_batch(seqs, quals)
    check_joint(eng, m["x"], seqs, refs, what=(model, "pipeline 3"), row_atol=1e-10)
    assert eng.last_timing()[2] == 0


def test_sequences_out_of_the_double_range_take_the_log_space_form():
    """lambda = 40: the long sequences leave the double range of the scaled-linear tables and go through the fused scan kernel,
    the short ones stay on the scaled-linear path: both forms in one call, 1e-10 on the sums (Rounding)"""
    recs = io.read_fastq(gpath("syn_L150_n8.fq"))
    short_s, short_q = batch((4, 9, 16, 24), seed=40, neg_every=0)
    seqs = short_s[:2] + [s for _, s, _ in recs][:3] + short_s[2:]
    quals = short_q[:2] + [q for _, _, q in recs][:3] + short_q[2:]
    eng = api.Engine(P1, PAR, 50, 30, 1e-4, 0.1, 0, 0)
    eng.set_option("group", 2)
    eng.load_batch(seqs, quals)
    x = eng.initial_params(40.0)
    refs = table_refs(oracle_with(P1, x), seqs, quals, x)
    check_joint(eng, x, seqs, refs, what="lambda 40", row_atol=1e-10)
    assert 2 <= eng.last_timing()[2] < len(seqs)


def test_a_sequence_without_any_parse_sits_on_node_0_and_letter_O():
    o = jc.joint_oracle(P1)
    eng = api.Engine(P1, PAR, 50, 30, 1e-4, 0.1, 0, 0)
    x, seqs, quals = cc.no_parse_inputs(jc.joint_params(eng), o.hmm())
    eng.load_batch(seqs, quals)
    refs = table_refs(oracle_with(P1, x), seqs, quals, x)
    assert refs[0] is None and refs[1] is not None
    counts, prof = check_joint(eng, x, seqs, refs, what="no parse", row_atol=1e-10)
    assert np.array_equal(prof[0], jc.no_parse_joint(len(seqs[0]), eng.n_node)) and counts[0, 0, 0, 1] == len(seqs[0])


# ---- groupings, streamed batches, and what a call leaves alone

def test_groupings_agree_counts_equal_the_scan_and_nothing_else_changes():
    lens = [int(v) for v in np.linspace(20, 160, 9)][::-1]
    lens[2], lens[6] = lens[6], lens[2]
    seqs, quals = batch(lens, seed=5)
    base = api.Engine(P1, PAR, 50, 30, 1e-4, 0.1, 0, 0)
    base.load_batch(seqs, quals)
    x = jc.joint_params(base)
    first = base.pair_posteriors(x, 0.0)
    ctx, node = base.context_profiles(x), base.node_profiles(x)
    res, en = base.scan(x)
    want_c, want = base.joint_profiles(x, profile=True)
    again = base._pair_lists(sum(len(r[0]) for r in first), np.concatenate([r[3] for r in first]))
    for a, b in zip(first, again):       # (the list of the last pair call is still the first call's)
        assert all(np.array_equal(u, v) for u, v in zip(a, b))
    for a, b in zip(ctx, base.context_profiles(x)):
        np.testing.assert_allclose(b, a, rtol=1e-10, atol=1e-14)
    for a, b in zip(node, base.node_profiles(x)):
        np.testing.assert_allclose(b, a, rtol=1e-10, atol=1e-14)
    res2, en2 = base.scan(x)
    np.testing.assert_allclose(en2, en, rtol=1e-10, atol=1e-14)
    assert [r["rss"] for r in res2] == [r["rss"] for r in res]
    np.testing.assert_allclose(base.joint_profiles(x), want_c, rtol=1e-10, atol=1e-14)      # (profile=False: the same counts)
    # the counts summed over the batch = the scan's expected emission counts of the single-base rows of theta
    hmm = jc.joint_oracle(P1).hmm()
    off = np.concatenate([[0], np.cumsum(hmm["theta_sizes"])])
    tot = want_c.sum(axis=(0, 2))
    for r, size in enumerate(hmm["theta_sizes"]):
        if size == 4:
            owners = [m for m in range(base.n_node) if hmm["theta_id"][m] == r]
            np.testing.assert_allclose(tot[owners, 1:].sum(axis=0), en[off[r]:off[r + 1]], rtol=1e-8, atol=1e-10, err_msg="row %d" % r)
    for opts in ((("group", 1),), (("group", 3),), (("max_resident", 4),), (("poison", 1),)):
        eng = api.Engine(P1, PAR, 50, 30, 1e-4, 0.1, 0, 0)
        for k, v in opts:
            eng.set_option(k, v)
        eng.load_batch(seqs, quals)
        got_c, got = eng.joint_profiles(x, profile=True)
        np.testing.assert_allclose(got_c, want_c, rtol=1e-10, atol=1e-13, err_msg=str(opts))
        for k, (g, w) in enumerate(zip(got, want)):
            assert g.shape == w.shape
            np.testing.assert_allclose(g, w, rtol=1e-10, atol=1e-14, err_msg=str((opts, k)))


def test_a_workgroup_of_the_log_space_form_takes_several_sequences():
    """pipeline 3 with option slots 3: log_scan_args asks for min(slots, n_seq) table slots and launches as many workgroups, so
    n_blocks = 3 workgroups take the n_seq = 9 unsorted sequences of L 20 .. 160 of the grouping test off the atomic counter;
    jnt.X and jnt.vec are indexed by blockIdx.x, the planes of the counts stage by launch position.  Against the table
    references, not against another grouping."""
    lens = [int(v) for v in np.linspace(20, 160, 9)][::-1]
    lens[2], lens[6] = lens[6], lens[2]
    seqs, quals = batch(lens, seed=5)
    eng = engine_with(P1, 50, PIPELINE3 + (("slots", 3),))
    eng.load_batch(seqs, quals)
    x = jc.joint_params(eng)
    refs = table_refs(oracle_with(P1, x), seqs, quals, x)
    check_joint(eng, x, seqs, refs, what="slots 3", row_atol=1e-10)
    assert sum(r is not None for r in refs) >= 8
    assert (eng.slot_status()["slots"], eng.n_seq) == (3, 9)
    assert eng.last_timing()[2] == 0


# ---- command line

def test_command_line_writes_the_logo_file(tmp_path):
    fq, model = gpath("positive_head6.fq"), gpath("trna_a.model")
    a1, lf, lf2 = str(tmp_path / "a.raw"), str(tmp_path / "logo.txt"), str(tmp_path / "logo2.txt")
    cli.main(["scan", "-f", fq, "-q", model, "--out1", a1, "--out-logo", lf])
    recs = io.read_fastq(fq)
    m = io.read_model(model)
    eng = io.engine_from_model(m)
    eng.load_batch([s for _, s, _ in recs], [q for _, _, q in recs])
    counts = eng.joint_profiles(m["x"])
    res, _ = eng.scan(m["x"])
    got = io.read_logo(lf)
    assert (got["n_used"], got["n_total"], got["names"]) == (len(recs), len(recs), eng.describe()["node"])
    # (the tables are summed with LDS atomics, so a run differs from another in the last bits)
    np.testing.assert_allclose(got["counts"], api.motif_logo(counts)["counts"], rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(got["occurrences"].sum(), sum(len(s) for _, s, _ in recs), rtol=1e-9)
    ex = sorted(r["exist_prob"] for r in res)
    cut = 0.5 * (ex[len(ex) // 2 - 1] + ex[len(ex) // 2])
    cli.main(["scan", "-f", fq, "-q", model, "--out1", a1, "--out-logo", lf2, "--logo-min-exist", repr(cut)])
    got2 = io.read_logo(lf2)
    use = np.array([1.0 if r["exist_prob"] >= cut else 0.0 for r in res])
    assert 0 < use.sum() < len(recs) and (got2["n_used"], got2["n_total"]) == (int(use.sum()), len(recs))
    np.testing.assert_allclose(got2["counts"], api.motif_logo(counts, use)["counts"], rtol=1e-9, atol=1e-12)
    assert sorted(p.name for p in tmp_path.iterdir()) == ["a.raw", "logo.txt", "logo2.txt"]


def test_calls_without_a_batch_or_an_output_are_refused():
    eng = api.Engine(P1, PAR, 50, 30, 1e-4, 0.1, 0, 0)
    lib = api.load_library()
    x = np.zeros(eng.n_param)
    out = np.zeros(35 * eng.n_node)
    dp = C.POINTER(C.c_double)
    assert lib.elemdp_joint_profile(eng._h, x.ctypes.data_as(dp), eng.n_param, out.ctypes.data_as(dp), None) == -4      # ELEMDP_ESTATE
    seqs, quals = batch((20,), seed=1)
    eng.load_batch(seqs, quals)
    assert lib.elemdp_joint_profile(eng._h, x.ctypes.data_as(dp), eng.n_param, None, None) == -1      # ELEMDP_EINVAL
