"""Structural context profiles on the GPU: Engine.context_profiles against brute-force enumeration with the
oracle on the tiny batch of tests/test_ctx_cpu.py, against the definitions over the oracle's tables and the engine's own pair
call at the shapes where the kernels have code of their own, across groupings and streamed batches, against the frequencies of
the sampler beyond enumeration, and through `scan --out-context`."""
import threading
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from oracle import pyoracle as po
from rnaelem_amd import api, cli, io
from tests import ctx_check as cc
from tests.pair_check import check_scan, n_workers, oracle_refs
from tests.sample_check import bound
from tests.test_ctx_cpu import CASES, LENGTHS, case_inputs
from tests.test_pair_posterior_gpu import perturbed
from tests.test_pair_shapes_gpu import P1, P2, PAR, batch, edge_batch, oracle_maker
from tests.util import gpath

pytestmark = pytest.mark.gpu

BULGE_MAX_L = 97       # the reference's bulge column (a Python loop over the items) only up to this length


def pool_map(make, fn, jobs):
    """[fn(o, job)] over a thread pool, one oracle of make() per thread (the oracle's C calls release the GIL)"""
    local = threading.local()

    def one(job):
        if not hasattr(local, "o"):
            local.o = make()
        return fn(local.o, job)

    with ThreadPoolExecutor(max_workers=n_workers()) as ex:
        return list(ex.map(one, jobs))


def table_refs(make, seqs, quals, x):
    order = sorted(range(len(seqs)), key=lambda k: -len(seqs[k]))
    got = pool_map(make, lambda o, k: cc.table_profile(o, seqs[k], quals[k], x, bulge=len(seqs[k]) <= BULGE_MAX_L), order)
    out = [None] * len(seqs)
    for k, v in zip(order, got):
        out[k] = v
    return out


def check_profiles(eng, x, seqs, refs, what="", no_rss=False, row_atol=1e-12):
    """every column against the table reference (B only where the reference has it, I only there too: it is U - H - B); L + R
    against the engine's own pair call; rows sum to 1 within row_atol; entries in [0, 1]; no parse or no structure: exactly O = 1"""
    prof = eng.context_profiles(x)
    pairs = eng.pair_posteriors(x, 0.0)
    assert len(prof) == len(seqs)
    for k, (g, ref) in enumerate(zip(prof, refs)):
        L = len(seqs[k])
        assert g.shape == (L, 7), (what, k)
        if ref is None or no_rss:
            assert np.array_equal(g, cc.exterior_only(L)), (what, k)
            continue
        full = not np.isnan(ref[:, 4]).any()
        cc.assert_profile(g, ref, what=(what, k, L), cols=range(7) if full else (0, 1, 2, 3, 6))
        if not full:       # (I + B = U - H where neither is clamped)
            np.testing.assert_allclose(g[:, 4] + g[:, 5], ref[:, 5], rtol=1e-8, atol=1e-10, err_msg=str((what, k, "B + I")))
        np.testing.assert_allclose(g[:, 1] + g[:, 2], 1.0 - pairs[k][3], rtol=0, atol=1e-10, err_msg=str((what, k, "L + R")))
        np.testing.assert_allclose(g.sum(axis=1), 1.0, rtol=0, atol=row_atol, err_msg=str((what, k, "row sums")))
        assert g.min() >= 0.0 and g.max() <= 1.0, (what, k)
    return prof


# ---- 5. the tiny batch against the enumeration

TINY = CASES      # every case of tests/test_ctx_cpu.py: three patterns, with and without energies, min_bpp 0 and 1e-4


@pytest.fixture(scope="module")
def tiny_refs():
    jobs = [(case, k) for case in TINY for k in range(len(LENGTHS))]
    inputs = {case: case_inputs(case) for case in TINY}

    def one(_, job):
        case, k = job
        pattern, flags, min_bpp = case
        x, seqs, quals = inputs[case]
        o = cc.ctx_oracle(pattern, 50, 30, min_bpp=min_bpp, flags=flags)
        o.set_params(x)
        return cc.enumerated_profile(o, seqs[k], quals[k])

    got = pool_map(lambda: None, one, jobs)
    return inputs, {job: e for job, e in zip(jobs, got)}


@pytest.mark.parametrize("opts", [(), (("fast", 0),), (("pipeline", 3),)], ids=["default", "fast0", "pipeline3"])
def test_tiny_batch_equals_the_enumeration(opts, tiny_refs):
    inputs, enum = tiny_refs
    top = np.zeros(7)
    for case in TINY:
        pattern, flags, min_bpp = case
        x, seqs, quals = inputs[case]
        eng = api.Engine(pattern, PAR, 50, 30, min_bpp, 0.1, flags, 0)
        for k, v in opts:
            eng.set_option(k, v)
        eng.load_batch(seqs, quals)
        prof = eng.context_profiles(x)
        for k, g in enumerate(prof):
            e = enum[(case, k)]
            assert e is not None
            cc.assert_profile(g, e, what=(opts, case, k))
            np.testing.assert_allclose(g.sum(axis=1), 1.0, rtol=0, atol=1e-12)
            top = np.maximum(top, g.max(axis=0))
        assert eng.last_timing()[2] == 0      # (no sequence handed on by the range check; pipeline 3 runs none)
    assert np.all(top > 1e-3), dict(zip(cc.LETTERS, top))


# ---- 6. shapes against the definitions over the oracle's tables and the engine's own pair call

SHAPE_LENS = (1, 2, 5, 49, 50, 51, 107, 131, 200)      # 1, 2, 5, W-1, W, W+1, 2W+7, 131, 200 at W = 50


def shape_batch(lens, seed, with_edge):
    seqs, quals = batch(lens, seed=seed)
    if with_edge:
        es, eq = edge_batch()
        seqs, quals = seqs + es, quals + eq
    return seqs, quals


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
        seqs, quals = shape_batch(lens, seed=1000 * W + len(pattern) + len(lens), with_edge=(lens is SHAPE_LENS))
        x = perturbed(engine_with(pattern, W))
        return seqs, quals, x, table_refs(oracle_maker_ctx(pattern, x, W), seqs, quals, x)
    return cached(("shape", pattern, W, lens), compute)


W20_LENS, W70_LENS, LONG_LENS = (5, 19, 20, 21, 47), (66, 70, 93), (257, 300)


@pytest.mark.parametrize("pattern,W,lens", [(P1, 50, SHAPE_LENS), (P2, 50, SHAPE_LENS), (P1, 20, W20_LENS), (P1, 50, LONG_LENS),
                                            (P1, 70, W70_LENS)], ids=["P1-W50", "P2-W50", "P1-W20", "P1-W50-long", "P1-W70"])
def test_shapes_against_the_table_definitions(pattern, W, lens):
    """(L = 257 and 300: k_ctx_seq forms its prefix sums per tile of 256 positions and carries them into the second tile; W = 70:
    spans above 64)"""
    seqs, quals, x, refs = shape_case(pattern, W, lens)
    eng = engine_with(pattern, W)
    eng.load_batch(seqs, quals)
    prof = check_profiles(eng, x, seqs, refs, what=(pattern, W))
    assert sum(r is not None for r in refs) >= len(lens)
    if lens is SHAPE_LENS:
        n0 = len(lens)
        for k in (n0 + 2, n0 + 4, n0 + 5, n0 + 7):           # all N, poly-A, L = 1, L = 2: no kept pair
            assert np.all(prof[k][:, 0] >= 1.0 - 1e-12), k
        assert max(p[:, 4].max() for p in prof) > 1e-2 and max(p[:, 5].max() for p in prof) > 1e-2


@pytest.mark.parametrize("W,lens", [(20, W20_LENS), (70, W70_LENS), (50, LONG_LENS)], ids=["P1-W20", "P1-W70", "P1-W50-long"])
def test_shapes_in_the_log_space_form(W, lens):
    """pipeline 3: k_dp<DP_SCAN> and CtxLog fill the planes of k_ctx_seq, addressed by launch position; the references of the
    scaled-linear cases, rows within 1e-10 (test_sequences_out_of_the_double_range_take_the_log_space_form)"""
    seqs, quals, x, refs = shape_case(P1, W, lens)
    eng = engine_with(P1, W, PIPELINE3)
    eng.load_batch(seqs, quals)
    check_profiles(eng, x, seqs, refs, what=(W, "pipeline 3"), row_atol=1e-10)
    assert sum(r is not None for r in refs) >= len(lens)
    assert eng.last_timing()[2] == 0


MODELS = ["syn_sm.model", "syn_a2007.model", "2.model"]


def model_case(model):
    def compute():
        m = io.read_model(gpath(model))
        seqs, quals = batch((3, 13, 40, 97, 131), seed=len(model))
        return m, seqs, quals, table_refs(lambda: cc.ctx_oracle_from_model(gpath(model))[0], seqs, quals, m["x"])
    return cached(("model", model), compute)


@pytest.mark.parametrize("model", MODELS)
def test_models_against_the_table_definitions(model):
    """softmax theta, the ~A2007~ energy parameters, and a model without secondary structure (2.model: O = 1 everywhere)"""
    m, seqs, quals, refs = model_case(model)
    eng = io.engine_from_model(m)
    eng.load_batch(seqs, quals)
    x = m["x"]
    prof = check_profiles(eng, x, seqs, refs, what=model, no_rss=m["no_rss"])
    if m["no_rss"]:
        assert all(np.array_equal(g, cc.exterior_only(len(s))) for g, s in zip(prof, seqs))


@pytest.mark.parametrize("model", MODELS)
def test_models_in_the_log_space_form(model):
    """pipeline 3 (2.model: the no_rss branches of k_dp, ctx.o = 1)"""
    m, seqs, quals, refs = model_case(model)
    eng = io.engine_from_model(m)
    eng.set_option("pipeline", 3)
    eng.load_batch(seqs, quals)
    x = m["x"]
    prof = check_profiles(eng, x, seqs, refs, what=(model, "pipeline 3"), no_rss=m["no_rss"], row_atol=1e-10)
    if m["no_rss"]:
        assert all(np.array_equal(g, cc.exterior_only(len(s))) for g, s in zip(prof, seqs))
    assert eng.last_timing()[2] == 0


def test_sequences_out_of_the_double_range_take_the_log_space_form():
    """lambda = 40: the long sequences leave the double range of the scaled-linear tables and go through the fused scan kernel
    in chunks of two (option group 2), the short ones stay on the scaled-linear path: both forms in one call.  Rows sum to 1
    within 1e-10 here, the project's tolerance of `unpaired`: in log space a term is exp(a + b - ln Z) with |ln Z| of a few
    thousand at this lambda, so the rounding of the exponent alone is eps * |ln Z| ~ 1e-12 relative per term, and where the
    remainder M would round below 0 its clamp leaves that excess in the row sum."""
    recs = io.read_fastq(gpath("syn_L150_n8.fq"))
    short_s, short_q = batch((4, 9, 16, 24), seed=40, neg_every=0)
    seqs = short_s[:2] + [s for _, s, _ in recs][:4] + short_s[2:]
    quals = short_q[:2] + [q for _, _, q in recs][:4] + short_q[2:]
    eng = api.Engine(P1, PAR, 50, 30, 1e-4, 0.1, 0, 0)
    eng.set_option("group", 2)
    eng.load_batch(seqs, quals)
    x = eng.initial_params(40.0)
    refs = table_refs(oracle_maker_ctx(P1, x), seqs, quals, x)
    check_profiles(eng, x, seqs, refs, what="lambda 40", row_atol=1e-10)
    eng.context_profiles(x)
    assert 3 <= eng.last_timing()[2] < len(seqs)


def test_a_sequence_without_any_parse_is_exactly_exterior():
    """theta(A) = -inf: poly-A has Z(ari, nasi) = 0 and gets O = 1 and zeros exactly; the sequence without A in the same group
    keeps its profile"""
    o = cc.ctx_oracle(P1)
    eng = api.Engine(P1, PAR, 50, 30, 1e-4, 0.1, 0, 0)
    x, seqs, quals = cc.no_parse_inputs(perturbed(eng), o.hmm())
    eng.load_batch(seqs, quals)
    refs = table_refs(oracle_maker_ctx(P1, x), seqs, quals, x)
    assert refs[0] is None and refs[1] is not None
    prof = check_profiles(eng, x, seqs, refs, what="no parse", row_atol=1e-10)
    assert np.array_equal(prof[0], cc.exterior_only(len(seqs[0])))


def oracle_maker_ctx(pattern, x, W=50, C=30):
    def make():
        o = cc.ctx_oracle(pattern, W, C)
        o.set_params(x)
        return o
    return make


# ---- 7. groupings

def test_groupings_agree_and_nothing_else_changes():
    lens = [int(v) for v in np.linspace(20, 280, 11)][::-1]
    lens[2], lens[7] = lens[7], lens[2]
    seqs, quals = batch(lens, seed=5)
    base = api.Engine(P1, PAR, 50, 30, 1e-4, 0.1, 0, 0)
    base.load_batch(seqs, quals)
    x = perturbed(base)
    first = base.pair_posteriors(x, 0.0)
    want = base.context_profiles(x)
    again = base._pair_lists(sum(len(r[0]) for r in first), np.concatenate([r[3] for r in first]))
    for a, b in zip(first, again):       # (the list of the last pair call is still the first call's)
        assert all(np.array_equal(u, v) for u, v in zip(a, b))
    refs = oracle_refs(oracle_maker(P1, 50, 30, x), seqs, quals)
    check_scan(base, x, seqs, refs)
    for opts in ((("group", 3),), (("group_streams", 1),), (("group_streams", 2),), (("max_resident", 4),)):
        eng = api.Engine(P1, PAR, 50, 30, 1e-4, 0.1, 0, 0)
        for k, v in opts:
            eng.set_option(k, v)
        eng.load_batch(seqs, quals)
        got = eng.context_profiles(x)
        for k, (g, w) in enumerate(zip(got, want)):
            np.testing.assert_allclose(g, w, rtol=1e-10, atol=1e-14, err_msg=str((opts, k)))


GROUPED_LENS = [int(v) for v in np.linspace(20, 280, 11)][::-1]
GROUPED_LENS[2], GROUPED_LENS[7] = GROUPED_LENS[7], GROUPED_LENS[2]      # (the lengths of the grouping test)


def test_a_workgroup_of_the_log_space_form_takes_several_sequences():
    """pipeline 3 with option slots 3: log_scan_args asks for min(slots, n_seq) table slots and launches as many workgroups, so
    n_blocks = 3 workgroups take the n_seq = 11 unsorted sequences of L 20 .. 280 off the atomic counter; the per-workgroup
    scratch is indexed by blockIdx.x, the planes of k_ctx_seq by launch position.  Against the table references, not against
    another grouping."""
    seqs, quals = batch(GROUPED_LENS, seed=5)
    eng = engine_with(P1, 50, PIPELINE3 + (("slots", 3),))
    eng.load_batch(seqs, quals)
    x = perturbed(eng)
    refs = table_refs(oracle_maker_ctx(P1, x), seqs, quals, x)
    check_profiles(eng, x, seqs, refs, what="slots 3", row_atol=1e-10)
    assert sum(r is not None for r in refs) >= 10
    assert (eng.slot_status()["slots"], eng.n_seq) == (3, 11)
    assert eng.last_timing()[2] == 0


# ---- 8. the split beyond enumeration

def test_letter_frequencies_of_the_sampler_lie_within_the_bound_of_the_profile():
    N = 4000
    seqs, quals = batch((40, 71, 100), seed=8, n_every=0)
    eng = api.Engine(P1, PAR, 50, 30, 1e-4, 0.1, 0, 0)
    eng.load_batch(seqs, quals)
    x = perturbed(eng)
    prof = eng.context_profiles(x)
    smp = eng.sample_structures(x, N, seed=3)
    for k, ((rss, _, _, st), g) in enumerate(zip(smp, prof)):
        assert st == eng.SAMPLED
        letters = np.frombuffer("".join(rss).encode(), dtype=np.uint8).reshape(N, len(seqs[k]))
        for c, ch in enumerate(cc.LETTERS):
            f = (letters == ord(ch)).mean(axis=0)
            bad = np.abs(f - g[:, c]) > bound(g[:, c], N)
            assert not bad.any(), (k, ch, [(int(p), f[p], g[p, c]) for p in np.nonzero(bad)[0][:5]])
    assert max(g[:, 4].max() for g in prof) > 0.05 and max(g[:, 5].max() for g in prof) > 0.05


# ---- 9. command line

def test_command_line_writes_the_context_file(tmp_path):
    fq, model = gpath("positive_head6.fq"), gpath("trna_a.model")
    a1, cf = str(tmp_path / "a.raw"), str(tmp_path / "ctx.txt")
    cli.main(["scan", "-f", fq, "-q", model, "--out1", a1, "--out-context", cf, "--out-pairs", str(tmp_path / "p.txt")])
    recs = io.read_fastq(fq)
    got = io.read_context_records(cf)
    assert [g[0] for g in got] == [r[0] for r in recs]
    assert len(io.read_pair_records(str(tmp_path / "p.txt"))) == len(recs)
    m = io.read_model(model)
    eng = io.engine_from_model(m)
    eng.load_batch([s for _, s, _ in recs], [q for _, _, q in recs])
    want = eng.context_profiles(m["x"])
    for (rid, g), w in zip(got, want):
        printed = np.array([[float(io.fmt(v)) for v in row] for row in w])
        # (the printed 6 digits; the tables are summed with LDS atomics, so a run differs from another in the last bits)
        np.testing.assert_allclose(g, printed, rtol=2e-6, atol=1e-12, err_msg=rid)


def test_calls_without_a_batch_or_an_output_are_refused():
    import ctypes as C
    eng = api.Engine(P1, PAR, 50, 30, 1e-4, 0.1, 0, 0)
    lib = api.load_library()
    x = np.zeros(eng.n_param)
    out = np.zeros(7)
    dp = C.POINTER(C.c_double)
    assert lib.elemdp_context_profile(eng._h, x.ctypes.data_as(dp), eng.n_param, out.ctypes.data_as(dp)) == -4      # ELEMDP_ESTATE
    seqs, quals = batch((20,), seed=1)
    eng.load_batch(seqs, quals)
    assert lib.elemdp_context_profile(eng._h, x.ctypes.data_as(dp), eng.n_param, None) == -1      # ELEMDP_EINVAL
