"""Accessibility on the GPU: Engine.accessibility against brute-force enumeration with the oracle on the
tiny batch of tests/test_access_cpu.py, against the path sums over the oracle's tables and the engine's own pair call at the
shapes where the kernels have code of their own, in both forms in one call, across groupings, streamed batches and poisoned
slots, next to the other calls of the handle, and through `scan --out-access`."""
import ctypes as C

import numpy as np
import pytest

from oracle import pyoracle as po
from rnaelem_amd import api, cli, io, synth
from tests import access_check as ac
from tests import ctx_check as cc
from tests.test_access_cpu import CASES, LENGTHS, U, case_inputs
from tests.test_ctx_gpu import pool_map
from tests.test_pair_posterior_gpu import perturbed
from tests.test_pair_shapes_gpu import P1, PAR, batch
from tests.util import gpath

pytestmark = pytest.mark.gpu

P5 = "(.....)"


def maker(pattern, x, W=50, C_=30, flags=0, min_bpp=1e-4):
    def make():
        o = ac.access_oracle(pattern, W, C_, min_bpp=min_bpp, flags=flags)
        o.set_params(x)
        return o
    return make


def table_refs(make, seqs, quals, x, width):
    """[(accessibility, terms) or None] per sequence, the longest first over a thread pool"""
    order = sorted(range(len(seqs)), key=lambda k: -len(seqs[k]))
    got = pool_map(make, lambda o, k: ac.table_access(o, seqs[k], quals[k], x, width), order)
    out = [None] * len(seqs)
    for k, v in zip(order, got):
        out[k] = v
    return out


def check_access(eng, x, seqs, refs, width, what="", atol=1e-10, unp_atol=1e-12, no_rss=False):
    """every window against the table reference (NaN exactly on the tail, values in [0, 1]); width 1 against the engine's own
    unpaired vector; a wider window never likelier than the two it holds; no parse or no structure: exactly 1"""
    acc = eng.accessibility(x, width)
    pairs = eng.pair_posteriors(x, 0.0)
    assert len(acc) == len(seqs)
    for k, (g, ref) in enumerate(zip(acc, refs)):
        L = len(seqs[k])
        assert g.shape == (L, width), (what, k)
        if ref is None or no_rss:
            assert np.array_equal(g, ac.all_ones(L, width), equal_nan=True), (what, k)
            continue
        ac.assert_access(g, ref[0], what=(what, k, L), atol=atol)
        if unp_atol is not None:
            np.testing.assert_allclose(g[:, 0], pairs[k][3], rtol=0, atol=unp_atol, err_msg=str((what, k, "width 1")))
        for w in range(1, width):
            n = L - w
            if n > 0:
                assert np.all(g[:n, w] <= np.minimum(g[:n, w - 1], g[1:n + 1, w - 1]) + 1e-12), (what, k, w)
    return acc


# ---- the tiny batch against the enumeration

@pytest.fixture(scope="module")
def tiny_refs():
    jobs = [(case, k) for case in CASES for k in range(len(LENGTHS))]
    inputs = {case: case_inputs(case) for case in CASES}

    def one(_, job):
        case, k = job
        pattern, flags, min_bpp = case
        x, seqs, quals = inputs[case]
        o = ac.access_oracle(pattern, 50, 30, min_bpp=min_bpp, flags=flags)
        o.set_params(x)
        return ac.enumerated_access(o, seqs[k], quals[k], U)

    got = pool_map(lambda: None, one, jobs)
    return inputs, {job: e for job, e in zip(jobs, got)}


@pytest.mark.parametrize("opts", [(), (("fast", 0),), (("pipeline", 3),)], ids=["default", "fast0", "pipeline3"])
def test_tiny_batch_equals_the_enumeration(opts, tiny_refs):
    inputs, enum = tiny_refs
    for case in CASES:
        pattern, flags, min_bpp = case
        x, seqs, quals = inputs[case]
        eng = api.Engine(pattern, PAR, 50, 30, min_bpp, 0.1, flags, 0)
        for k, v in opts:
            eng.set_option(k, v)
        eng.load_batch(seqs, quals)
        for k, g in enumerate(eng.accessibility(x, U)):
            e = enum[(case, k)]
            assert e is not None
            ac.assert_access(g, e, what=(opts, case, k))
        assert eng.last_timing()[2] == 0      # (no sequence handed on by the range check; pipeline 3 runs none)


# ---- shapes against the path sums over the oracle's tables and the engine's own pair call

RAGGED = (1, 2, 5, 13, 40, 97, 131, 200)


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


def shape_case(pattern, W, lens, width):
    """(seqs, quals, x, table references) of a shape case"""
    def compute():
        seqs, quals = batch(lens, seed=1000 * W + len(pattern) + len(lens), n_every=3 if len(lens) > 1 else 0, neg_every=2)
        x = perturbed(engine_with(pattern, W))
        return seqs, quals, x, table_refs(maker(pattern, x, W), seqs, quals, x, width)
    return cached(("shape", pattern, W, lens, width), compute)


W20_LENS, W70_LENS, LONG_LENS = (5, 19, 20, 21, 47), (66, 70, 93), (257, 300)


@pytest.mark.parametrize("pattern,W,lens,width", [(P1, 50, RAGGED, 16), (P5, 50, RAGGED, 16), (P1, 20, W20_LENS, 16),
                                                  (P1, 50, LONG_LENS, 16), (P1, 50, (40,), 1), (P1, 50, (40,), 64),
                                                  (P1, 70, W70_LENS, 16)],
                         ids=["P1-W50", "P5-W50", "P1-W20", "P1-W50-long", "U1", "U64", "P1-W70"])
def test_shapes_against_the_table_path_sums(pattern, W, lens, width):
    """(L = 257 and 300: more windows than one tile of k_access_seq, more positions than one row of workgroups of the chain
    kernel's first 256 units; U = 64 at L = 40: every width a lane of the T_L scan, most windows off the end; W = 70: spans
    above 64)"""
    seqs, quals, x, refs = shape_case(pattern, W, lens, width)
    eng = engine_with(pattern, W)
    eng.load_batch(seqs, quals)
    assert all(r is not None for r in refs)
    check_access(eng, x, seqs, refs, width, what=(pattern, W, width))
    assert eng.last_timing()[2] == 0


@pytest.mark.parametrize("W,lens", [(20, W20_LENS), (70, W70_LENS), (50, LONG_LENS)], ids=["P1-W20", "P1-W70", "P1-W50-long"])
def test_shapes_in_the_log_space_form(W, lens):
    """pipeline 3: k_dp<DP_SCAN> and access_log_units (AccLog, the lanes' state vectors in acc.vec) fill the term planes
    k_access_seq sums, addressed by launch position; the references of the scaled-linear cases at the 1e-10 of
    test_sequences_out_of_the_double_range_take_the_log_space_form"""
    seqs, quals, x, refs = shape_case(P1, W, lens, 16)
    eng = engine_with(P1, W, PIPELINE3)
    eng.load_batch(seqs, quals)
    assert all(r is not None for r in refs)
    check_access(eng, x, seqs, refs, 16, what=(W, "pipeline 3"), atol=1e-10, unp_atol=1e-10)
    assert eng.last_timing()[2] == 0


def test_a_model_without_energies_carries_both_multi_loop_terms():
    """with energies the two multi-loop terms are ~1e-8 and the absolute tolerance would hide a wrong one; without them the
    reference has both at 1e-3 or more.  (No comparison with `unpaired` of the pair call here: without energies the interior
    loops of more than max_iloop bases that the outside pass enumerates and the inside pass does not weigh 2.5e-7 at L = 40,
    in the oracle's own tables too -- 1 - sum P and the path sums cut the derivations at different items.  At max_iloop 50 the
    two agree to 3e-14.)"""
    (s,), (q,) = synth.synth_batch(1, 40, seed=140)
    (s2,), (q2,) = synth.synth_batch(1, 33, seed=133)
    seqs, quals = [s, s2], [q, q2]
    top = {"2": 0.0, "M": 0.0}
    for pattern in ("(.*)", P1):
        eng = api.Engine(pattern, PAR, 50, 30, 0.0, 0.1, po.NO_ENE, 0)
        eng.load_batch(seqs, quals)
        x = perturbed(eng)
        refs = table_refs(maker(pattern, x, flags=po.NO_ENE, min_bpp=0.0), seqs, quals, x, 16)
        for r in refs:
            for k in top:
                top[k] = max(top[k], float(r[1][k].max()))
        check_access(eng, x, seqs, refs, 16, what=(pattern, "no_ene"), unp_atol=None)
    assert top["2"] >= 1e-3 and top["M"] >= 1e-3, top


MODELS = ["syn_sm.model", "syn_a2007.model", "2.model"]


def model_case(model):
    def compute():
        m = io.read_model(gpath(model))
        seqs, quals = batch((3, 13, 40, 97), seed=len(model))
        return m, seqs, quals, table_refs(lambda: ac.access_oracle_from_model(gpath(model))[0], seqs, quals, m["x"], 16)
    return cached(("model", model), compute)


@pytest.mark.parametrize("model", MODELS)
def test_models_against_the_table_path_sums(model):
    """softmax theta, the ~A2007~ energy parameters, and a model without secondary structure (2.model: 1 in every valid window)"""
    m, seqs, quals, refs = model_case(model)
    eng = io.engine_from_model(m)
    eng.load_batch(seqs, quals)
    check_access(eng, m["x"], seqs, refs, 16, what=model, no_rss=m["no_rss"])


@pytest.mark.parametrize("model", MODELS)
def test_models_in_the_log_space_form(model):
    """pipeline 3 (2.model: the no_rss branches of k_dp, access_log_units skipped)"""
    m, seqs, quals, refs = model_case(model)
    eng = io.engine_from_model(m)
    eng.set_option("pipeline", 3)
    eng.load_batch(seqs, quals)
    check_access(eng, m["x"], seqs, refs, 16, what=(model, "pipeline 3"), atol=1e-10, unp_atol=1e-10, no_rss=m["no_rss"])
    assert eng.last_timing()[2] == 0


def test_sequences_out_of_the_double_range_take_the_log_space_form():
    """lambda = 40: the long sequences leave the double range of the scaled-linear tables and go through the fused scan kernel,
    the short ones stay on the scaled-linear path: both forms in one call.  1e-10 here: in log space a term is
    exp(a + b - ln Z) with |ln Z| of a few thousand at this lambda, so the exponent alone rounds at eps |ln Z| ~ 1e-12 relative
    per term."""
    recs = io.read_fastq(gpath("syn_L150_n8.fq"))
    short_s, short_q = batch((4, 9, 16, 24), seed=40, neg_every=0)
    seqs = short_s[:2] + [s for _, s, _ in recs][:3] + short_s[2:]
    quals = short_q[:2] + [q for _, _, q in recs][:3] + short_q[2:]
    eng = api.Engine(P1, PAR, 50, 30, 1e-4, 0.1, 0, 0)
    eng.set_option("group", 2)
    eng.load_batch(seqs, quals)
    x = eng.initial_params(40.0)
    refs = table_refs(maker(P1, x), seqs, quals, x, 16)
    check_access(eng, x, seqs, refs, 16, what="lambda 40", atol=1e-10, unp_atol=1e-10)
    eng.accessibility(x, 16)
    assert 1 <= eng.last_timing()[2] < len(seqs)


def test_a_sequence_without_any_parse_is_exactly_one():
    """theta(A) = -inf: poly-A has Z(ari, nasi) = 0 and gets 1 in every valid window exactly; the sequence without A in the same
    group keeps its values"""
    o = ac.access_oracle(P1)
    eng = api.Engine(P1, PAR, 50, 30, 1e-4, 0.1, 0, 0)
    x, seqs, quals = cc.no_parse_inputs(perturbed(eng), o.hmm())
    eng.load_batch(seqs, quals)
    refs = table_refs(maker(P1, x), seqs, quals, x, 16)
    assert refs[0] is None and refs[1] is not None
    acc = check_access(eng, x, seqs, refs, 16, what="no parse")
    assert np.array_equal(acc[0], ac.all_ones(len(seqs[0]), 16), equal_nan=True)


# ---- groupings, streamed batches, poisoned slots; the other calls of the handle

def test_groupings_agree_and_nothing_else_changes():
    lens = [int(v) for v in np.linspace(20, 280, 9)][::-1]
    lens[2], lens[6] = lens[6], lens[2]
    seqs, quals = batch(lens, seed=5)
    base = api.Engine(P1, PAR, 50, 30, 1e-4, 0.1, 0, 0)
    base.load_batch(seqs, quals)
    x = perturbed(base)
    first = base.pair_posteriors(x, 0.0)
    ctx0 = base.context_profiles(x)
    want = base.accessibility(x, 16)
    again = base._pair_lists(sum(len(r[0]) for r in first), np.concatenate([r[3] for r in first]))
    for a, b in zip(first, again):       # (the list of the last pair call is still the first call's)
        assert all(np.array_equal(u, v) for u, v in zip(a, b))
    second = base.pair_posteriors(x, 0.0)
    for a, b in zip(first, second):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        np.testing.assert_allclose(a[2], b[2], rtol=1e-10, atol=1e-14)
    for a, b in zip(ctx0, base.context_profiles(x)):
        np.testing.assert_allclose(a, b, rtol=1e-10, atol=1e-14)
    recs0, _ = base.scan(x)
    for g, w in zip(base.accessibility(x, 16), want):      # (and the call itself behind a scan)
        np.testing.assert_allclose(g, w, rtol=1e-10, atol=1e-14)
    for opts in ((("group", 1),), (("group", 3),), (("max_resident", 4),), (("poison", 1),)):
        eng = api.Engine(P1, PAR, 50, 30, 1e-4, 0.1, 0, 0)
        for k, v in opts:
            eng.set_option(k, v)
        eng.load_batch(seqs, quals)
        got = eng.accessibility(x, 16)
        for k, (g, w) in enumerate(zip(got, want)):
            assert g.shape == w.shape and np.array_equal(np.isnan(g), np.isnan(w)), (opts, k)
            np.testing.assert_allclose(g, w, rtol=1e-10, atol=1e-14, err_msg=str((opts, k)))


# ---- command line, refusals

def test_a_workgroup_of_the_log_space_form_takes_several_sequences():
    """pipeline 3 with option slots 3: log_scan_args asks for min(slots, n_seq) table slots and launches as many workgroups, so
    n_blocks = 3 workgroups take the n_seq = 9 unsorted sequences of L 20 .. 280 of the grouping test off the atomic counter;
    acc.vec is indexed by blockIdx.x, the term planes by launch position.  Against the table references, not against another
    grouping."""
    lens = [int(v) for v in np.linspace(20, 280, 9)][::-1]
    lens[2], lens[6] = lens[6], lens[2]
    seqs, quals = batch(lens, seed=5)
    eng = engine_with(P1, 50, PIPELINE3 + (("slots", 3),))
    eng.load_batch(seqs, quals)
    x = perturbed(eng)
    refs = table_refs(maker(P1, x), seqs, quals, x, 16)
    assert sum(r is not None for r in refs) >= 8
    check_access(eng, x, seqs, refs, 16, what="slots 3", atol=1e-10, unp_atol=1e-10)
    assert (eng.slot_status()["slots"], eng.n_seq) == (3, 9)
    assert eng.last_timing()[2] == 0


def test_command_line_writes_the_access_file(tmp_path):
    fq, model = gpath("positive_head6.fq"), gpath("trna_a.model")
    a1, af = str(tmp_path / "a.raw"), str(tmp_path / "access.txt")
    cli.main(["scan", "-f", fq, "-q", model, "--out1", a1, "--out-access", af, "--access-width", "8", "--out-pairs", str(tmp_path / "p.txt")])
    recs = io.read_fastq(fq)
    got = io.read_access_records(af)
    assert [g[0] for g in got] == [r[0] for r in recs]
    assert len(io.read_pair_records(str(tmp_path / "p.txt"))) == len(recs)
    m = io.read_model(model)
    eng = io.engine_from_model(m)
    eng.load_batch([s for _, s, _ in recs], [q for _, _, q in recs])
    want = eng.accessibility(m["x"], 8)
    for (rid, g), w in zip(got, want):
        assert g.shape == w.shape and np.array_equal(np.isnan(g), np.isnan(w)), rid
        printed = np.array([[float(io.fmt(v)) for v in row] for row in w])
        # (the printed 6 digits; the tables are summed with LDS atomics, so a run differs from another in the last bits)
        np.testing.assert_allclose(g, printed, rtol=2e-6, atol=1e-12, err_msg=rid)


def test_calls_without_a_batch_or_with_bad_arguments_are_refused():
    eng = api.Engine(P1, PAR, 50, 30, 1e-4, 0.1, 0, 0)
    lib = api.load_library()
    x = np.zeros(eng.n_param)
    out = np.zeros(64 * 20)
    dp = C.POINTER(C.c_double)
    xp, op = x.ctypes.data_as(dp), out.ctypes.data_as(dp)
    assert lib.elemdp_accessibility(eng._h, xp, eng.n_param, 16, op) == -4      # ELEMDP_ESTATE
    seqs, quals = batch((20,), seed=1)
    eng.load_batch(seqs, quals)
    assert lib.elemdp_accessibility(eng._h, xp, eng.n_param, 16, None) == -1    # ELEMDP_EINVAL
    assert lib.elemdp_accessibility(eng._h, None, eng.n_param, 16, op) == -1
    assert lib.elemdp_accessibility(eng._h, xp, eng.n_param, 0, op) == -1
    assert lib.elemdp_accessibility(eng._h, xp, eng.n_param, 65, op) == -1
    assert lib.elemdp_accessibility(eng._h, xp, eng.n_param, 64, op) == 0


def test_option_access_terms_gives_the_parts_of_the_sum():
    """the four terms one at a time against the reference's terms, and their sum against the whole call"""
    (s,), (q,) = synth.synth_batch(1, 40, seed=140)
    eng = api.Engine("(.*)", PAR, 50, 30, 0.0, 0.1, po.NO_ENE, 0)
    eng.load_batch([s], [q])
    x = perturbed(eng)
    ref = table_refs(maker("(.*)", x, flags=po.NO_ENE, min_bpp=0.0), [s], [q], x, 16)[0]
    valid = ~ac.nan_tail(40, 16)
    for bit, name in enumerate(ac.TERMS):
        eng.set_option("access_terms", 1 << bit)
        (g,) = eng.accessibility(x, 16)
        np.testing.assert_allclose(g[valid], ref[1][name][valid], rtol=1e-8, atol=1e-10, err_msg=name)
    eng.set_option("access_terms", 15)
    ac.assert_access(eng.accessibility(x, 16)[0], ref[0])
    with pytest.raises(api.ElemdpError):
        eng.set_option("access_terms", 16)
