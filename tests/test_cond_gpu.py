"""Motif-conditional pair posteriors on the GPU: Engine.conditional_pairs against brute-force enumeration
with the oracle on the tiny batch of tests/test_ctx_cpu.py, against the oracle's tables of both worlds and the engine's own pair
call (the mixture identity) at the shapes where the kernels have code of their own, on models, in the log-space form, on empty
worlds, across groupings, with poisoned table slots, next to the other calls of the handle, and through `scan --out-contrast`."""
import ctypes as C

import numpy as np
import pytest

from rnaelem_amd import api, cli, io
from tests import cond_check as cd
from tests import ctx_check as cc
from tests.test_cond_cpu import references
from tests.test_ctx_cpu import CASES
from tests.test_ctx_gpu import SHAPE_LENS, pool_map, shape_batch
from tests.test_pair_posterior_gpu import perturbed
from tests.test_pair_shapes_gpu import P1, P2, PAR, batch
from tests.util import gpath

pytestmark = pytest.mark.gpu

GAMMA = 1.0


def table_refs(pair_of_oracles, seqs, quals):
    """cond_check.table_worlds of every sequence over a thread pool; pair_of_oracles() makes a thread's two oracles"""
    order = sorted(range(len(seqs)), key=lambda k: -len(seqs[k]))
    got = pool_map(pair_of_oracles, lambda oo, k: cd.table_worlds(oo[0], oo[1], seqs[k], quals[k]), order)
    out = [None] * len(seqs)
    for k, v in zip(order, got):
        out[k] = v
    return out


def pattern_oracles(pattern, x, W=50, C=30):
    return lambda: cd.world_oracles(lambda: cc.ctx_oracle(pattern, W, C), x)


def check_batch(eng, x, seqs, refs, what="", enumerated=False, mixture=True):
    """conditional_pairs(x, 0, GAMMA) of the resident batch: every record against its reference, both structures against the
    mirror on the record's own numbers, and the mixture identity against the engine's own pair call"""
    recs = eng.conditional_pairs(x, 0.0, GAMMA)
    pairs = eng.pair_posteriors(x, 0.0) if mixture else None
    assert len(recs) == len(seqs)
    for k, (rec, ref) in enumerate(zip(recs, refs)):
        L, W = len(seqs[k]), min(len(seqs[k]), eng.max_span)
        cd.check_record(rec, ref, L, W, what=(what, k, L), enumerated=enumerated)
        cd.check_structures(rec, L, W, GAMMA, what=(what, k, L))
        if mixture:
            cd.check_mixture(rec, pairs[k], L, W, what=(what, k, L))
    return recs


def assert_comparable(refs, what=""):
    """of the sequences with a parse that has the motif, at least half have exist_prob >= E_MIN (P_motif is compared there; the
    sequences without such a parse -- too short for the pattern, or marked as without motif -- have P_motif = 0 exactly)"""
    es = [r["e"] for r in refs if np.isfinite(r["Zari"])]
    assert es and 2 * sum(e >= cd.E_MIN for e in es) >= len(es), (what, es)


# ---- 1. the tiny batch against the enumeration

@pytest.mark.parametrize("opts", [(), (("fast", 0),), (("pipeline", 3),)], ids=["default", "fast0", "pipeline3"])
def test_tiny_batch_equals_the_enumeration(opts):
    shifts = []
    for case in CASES:
        pattern, flags, min_bpp = case
        x, seqs, quals, enum, tab = references(case)
        eng = api.Engine(pattern, PAR, 50, 30, min_bpp, 0.1, flags, 0)
        for k, v in opts:
            eng.set_option(k, v)
        eng.load_batch(seqs, quals)
        recs = check_batch(eng, x, seqs, enum, what=(opts, case), enumerated=True, mixture=False)
        if not any(k == "pipeline" for k, _ in opts):
            assert eng.last_timing()[2] == 0      # (no sequence handed on by the range check)
        shifts += [r["shift"] for r in recs]
        assert all(1e-3 < r["exist_prob"] < 1.0 - 1e-3 for r in recs)
    assert max(shifts) > 0.1      # (the worlds differ: a swap, or Z(ari, nasi) as a normaliser, cannot pass)


# ---- 2. shapes against the oracle's tables and the engine's own pair call

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
    """(seqs, quals, x, the tables of both worlds) of a shape case"""
    def compute():
        seqs, quals = shape_batch(lens, seed=1000 * W + len(pattern) + len(lens), with_edge=(lens is SHAPE_LENS))
        x = perturbed(engine_with(pattern, W))
        return seqs, quals, x, table_refs(pattern_oracles(pattern, x, W), seqs, quals)
    return cached(("shape", pattern, W, lens), compute)


W20_LENS, W70_LENS, LONG_LENS = (5, 19, 20, 21, 47), (66, 70, 93), (257, 300)


@pytest.mark.parametrize("pattern,W,lens", [(P1, 50, SHAPE_LENS), (P2, 50, SHAPE_LENS), (P1, 20, W20_LENS), (P1, 50, LONG_LENS),
                                            (P1, 70, W70_LENS)], ids=["P1-W50", "P2-W50", "P1-W20", "P1-W50-long", "P1-W70"])
def test_shapes_against_the_tables_and_the_mixture(pattern, W, lens):
    """(L = 257 and 300: k_cond_seq walks the rows in tiles of 256 and carries the shift and the list position into the second;
    W = 70: spans above 64)"""
    seqs, quals, x, refs = shape_case(pattern, W, lens)
    eng = engine_with(pattern, W)
    eng.load_batch(seqs, quals)
    assert_comparable(refs, (pattern, W))
    if pattern == P1 and lens is SHAPE_LENS:
        # (here the world without the motif is a sliver of the mixture, and its P is still checked at full tolerance)
        assert any(np.isfinite(r["Znasi"]) and 0.0 < 1.0 - r["e"] < 1e-3 for r in refs), [r["e"] for r in refs]
    recs = check_batch(eng, x, seqs, refs, what=(pattern, W))
    assert eng.last_timing()[2] == 0
    if lens is SHAPE_LENS:
        n0 = len(lens)
        for k in (n0 + 2, n0 + 4, n0 + 5, n0 + 7):           # all N, poly-A, L = 1, L = 2: no kept pair
            assert len(recs[k]["i"]) == 0 and np.all(recs[k]["unpaired_none"] == 1.0), k


@pytest.mark.parametrize("W,lens", [(20, W20_LENS), (70, W70_LENS), (50, LONG_LENS)], ids=["P1-W20", "P1-W70", "P1-W50-long"])
def test_shapes_in_the_log_space_form(W, lens):
    """pipeline 3: k_dp<DP_SCAN> runs the two worlds in its loop over cond_p0 / cond_p1 and k_cond_seq reads their planes by
    launch position; the references and the checks of the scaled-linear cases"""
    seqs, quals, x, refs = shape_case(P1, W, lens)
    eng = engine_with(P1, W, PIPELINE3)
    eng.load_batch(seqs, quals)
    assert_comparable(refs, (P1, W))
    check_batch(eng, x, seqs, refs, what=(W, "pipeline 3"))
    assert eng.last_timing()[2] == 0


# ---- 3. models

MODELS = ["syn_sm.model", "syn_a2007.model", "2.model"]


def model_case(model):
    def compute():
        m = io.read_model(gpath(model))
        seqs, quals = batch((3, 13, 40, 97, 131), seed=len(model))
        return m, seqs, quals, table_refs(lambda: cd.model_oracles(gpath(model)), seqs, quals)
    return cached(("model", model), compute)


def check_model(model, opts):
    m, seqs, quals, refs = model_case(model)
    eng = io.engine_from_model(m)
    for k, v in opts:
        eng.set_option(k, v)
    eng.load_batch(seqs, quals)
    recs = check_batch(eng, m["x"], seqs, refs, what=(model, opts))
    if m["no_rss"]:
        for rec, s, ref in zip(recs, seqs, refs):
            assert len(rec["i"]) == 0 and np.all(rec["unpaired_motif"] == 1.0) and np.all(rec["unpaired_none"] == 1.0)
            assert rec["structure_motif"] == rec["structure_none"] == "." * len(s)
            if np.isfinite(ref["Zari"]) and np.isfinite(ref["Znasi"]):
                assert rec["shift"] == 0.0
    return eng


@pytest.mark.parametrize("model", MODELS)
def test_models_against_the_tables(model):
    """softmax theta, the ~A2007~ energy parameters, and a model without secondary structure (2.model: empty lists, unpaired 1,
    shift 0)"""
    check_model(model, ())


@pytest.mark.parametrize("model", MODELS)
def test_models_in_the_log_space_form(model):
    """pipeline 3 (2.model: the no_rss branches of k_dp, both worlds without pairs)"""
    eng = check_model(model, PIPELINE3)
    assert eng.last_timing()[2] == 0


# ---- 4. the log-space form

def test_sequences_out_of_the_double_range_take_the_log_space_form():
    """lambda = 40: the long sequences leave the double range of the scaled-linear tables and go through the fused scan kernel in
    chunks of two (option group 2), the short ones stay on the scaled-linear path: both forms in one call"""
    recs = io.read_fastq(gpath("syn_L150_n8.fq"))
    short_s, short_q = batch((4, 9, 16, 24), seed=40, neg_every=0)
    seqs = short_s[:2] + [s for _, s, _ in recs][:4] + short_s[2:]
    quals = short_q[:2] + [q for _, _, q in recs][:4] + short_q[2:]
    eng = api.Engine(P1, PAR, 50, 30, 1e-4, 0.1, 0, 0)
    eng.set_option("group", 2)
    eng.load_batch(seqs, quals)
    x = eng.initial_params(40.0)
    refs = table_refs(pattern_oracles(P1, x), seqs, quals)
    eng.conditional_pairs(x, 0.0)
    assert 3 <= eng.last_timing()[2] < len(seqs)
    check_batch(eng, x, seqs, refs, what="lambda 40")


# ---- 5. empty worlds

def test_a_sequence_without_any_parse_has_two_empty_worlds():
    """theta(A) = -inf: poly-A has Z(ari, nasi) = 0 -- P = 0, unpaired = 1, open structures, exist_prob 0 and shift NaN; the
    sequence without A in the same group keeps both of its worlds"""
    o = cc.ctx_oracle(P1)
    eng = api.Engine(P1, PAR, 50, 30, 1e-4, 0.1, 0, 0)
    x, seqs, quals = cc.no_parse_inputs(perturbed(eng), o.hmm())
    eng.load_batch(seqs, quals)
    refs = table_refs(pattern_oracles(P1, x), seqs, quals)
    assert not np.isfinite(refs[0]["Zo"]) and np.isfinite(refs[1]["Zari"]) and np.isfinite(refs[1]["Znasi"])
    recs = check_batch(eng, x, seqs, refs, what="no parse")
    r = recs[0]
    assert r["exist_prob"] == 0.0 and np.isnan(r["shift"]) and np.all(r["p_motif"] == 0.0) and np.all(r["p_none"] == 0.0)
    assert np.all(r["unpaired_motif"] == 1.0) and np.all(r["unpaired_none"] == 1.0)
    assert r["structure_motif"] == r["structure_none"] == "." * len(seqs[0])


def test_without_the_pattern_rows_the_motif_world_is_empty():
    """every pattern row of theta at -inf: no parse has the motif -- exist_prob 0.0 and P_motif = 0 exactly, and P_none is the
    engine's own pair posterior"""
    seqs, quals = batch((20, 47, 120), seed=9, neg_every=0)
    eng = api.Engine(P1, PAR, 50, 30, 1e-4, 0.1, 0, 0)
    eng.load_batch(seqs, quals)
    x = cd.none_params(perturbed(eng), eng.describe())
    refs = table_refs(pattern_oracles(P1, x), seqs, quals)
    recs = check_batch(eng, x, seqs, refs, what="no motif")
    pairs = eng.pair_posteriors(x, 0.0)
    for rec, pr, s in zip(recs, pairs, seqs):
        assert rec["exist_prob"] == 0.0 and np.all(rec["p_motif"] == 0.0) and np.all(rec["unpaired_motif"] == 1.0)
        assert rec["structure_motif"] == "." * len(s) and np.isnan(rec["shift"])
        np.testing.assert_allclose(rec["p_none"], pr[2], rtol=1e-8, atol=1e-12)
    assert max(rec["p_none"].max() for rec in recs) > 0.1


# ---- 6. / 7. groupings, poisoned table slots

@pytest.fixture(scope="module")
def grouped():
    lens = [int(v) for v in np.linspace(20, 280, 11)][::-1]
    lens[2], lens[7] = lens[7], lens[2]
    seqs, quals = batch(lens, seed=5)
    base = api.Engine(P1, PAR, 50, 30, 1e-4, 0.1, 0, 0)
    base.load_batch(seqs, quals)
    x = perturbed(base)
    return seqs, quals, x, base.conditional_pairs(x, 0.0, GAMMA)


@pytest.mark.parametrize("opts", [(("group", 3),), (("group_streams", 1),), (("group_streams", 2),), (("max_resident", 4),), (("poison", 1),)],
                         ids=lambda o: "%s-%d" % o[0])
def test_groupings_and_poisoned_slots_give_the_same_records(opts, grouped):
    """(the sweeps gather through LDS atomics: two runs agree to rounding.  poison 1: the table slots hold NaN before the sweeps,
    so an entry the nasi sweep did not write and the reduction read would show up)"""
    seqs, quals, x, want = grouped
    eng = api.Engine(P1, PAR, 50, 30, 1e-4, 0.1, 0, 0)
    for k, v in opts:
        eng.set_option(k, v)
    eng.load_batch(seqs, quals)
    got = eng.conditional_pairs(x, 0.0, GAMMA)
    for r in got:
        assert all(np.all(np.isfinite(r[key])) for key in ("p_motif", "p_none", "unpaired_motif", "unpaired_none"))
    cd.same_records(got, want, rtol=1e-10, atol=1e-14)


def test_a_workgroup_of_the_log_space_form_takes_several_sequences():
    """pipeline 3 with option slots 3: log_scan_args asks for min(slots, n_seq) table slots and launches as many workgroups, so
    n_blocks = 3 workgroups take the n_seq = 11 unsorted sequences of L 20 .. 280 of the grouping tests off the atomic counter.
    Against the oracle's tables of both worlds, not against another grouping."""
    lens = [int(v) for v in np.linspace(20, 280, 11)][::-1]
    lens[2], lens[7] = lens[7], lens[2]
    seqs, quals = batch(lens, seed=5)
    eng = engine_with(P1, 50, PIPELINE3 + (("slots", 3),))
    eng.load_batch(seqs, quals)
    x = perturbed(eng)
    refs = table_refs(pattern_oracles(P1, x), seqs, quals)
    assert_comparable(refs, "slots 3")
    check_batch(eng, x, seqs, refs, what="slots 3")
    assert (eng.slot_status()["slots"], eng.n_seq) == (3, 11)
    assert eng.last_timing()[2] == 0


# ---- 8. the other calls of the handle

def test_other_calls_are_untouched():
    """scan, pair_posteriors + pair_list, context_profiles, node_profiles and sample_structures before and after a conditional
    call on the same handle.  What stays on the device -- the list of the last pair call -- is the same bit for bit, and so is
    everything discrete that the calls return anew.  The floating results of a call that runs again agree to rounding only, with or
    without a conditional call in between: the sum passes gather through LDS atomics, so two runs of one call differ in the last
    bits (measured here: exist_prob 0.9966020858218474 against 0.9966020858218475)."""
    seqs, quals = batch((30, 61, 100), seed=12, neg_every=0)
    eng = api.Engine(P1, PAR, 50, 30, 1e-4, 0.1, 0, 0)
    eng.load_batch(seqs, quals)
    x = perturbed(eng)
    tol = dict(rtol=1e-10, atol=1e-12)

    def everything():
        scan, en = eng.scan(x)
        return dict(scan=scan, en=en, pairs=eng.pair_posteriors(x, 1e-3), ctx=eng.context_profiles(x), nodes=eng.node_profiles(x),
                    samples=eng.sample_structures(x, 20, seed=3))

    eng.train_eval(x)
    eng.seq_counts()
    before = everything()
    n_list = sum(len(r[0]) for r in before["pairs"])
    unp = np.concatenate([r[3] for r in before["pairs"]])
    eng.conditional_pairs(x, 1e-2, GAMMA)
    with pytest.raises(api.ElemdpError) as err:      # (as after any scan-family call)
        eng.seq_counts()
    assert err.value.code == -4
    # the list of the last pair call is still on the device, bit for bit
    for a, b in zip(before["pairs"], eng._pair_lists(n_list, unp)):
        assert all(np.array_equal(u, v) for u, v in zip(a, b))
    after = everything()
    for a, b in zip(before["scan"], after["scan"]):
        assert a["rss"] == b["rss"] and (a["Ys"], a["Ye"]) == (b["Ys"], b["Ye"]) and np.array_equal(a["psihat"], b["psihat"])
        np.testing.assert_allclose(b["exist_prob"], a["exist_prob"], **tol)
        for key in ("start", "inner", "end"):      # (log posteriors: rounding of the linear values is an absolute error here)
            np.testing.assert_allclose(b[key], a[key], **tol)
    np.testing.assert_allclose(after["en"], before["en"], **tol)
    for a, b in zip(before["pairs"], after["pairs"]):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        np.testing.assert_allclose(b[2], a[2], **tol)
        np.testing.assert_allclose(b[3], a[3], **tol)
    for key in ("ctx", "nodes"):
        for a, b in zip(before[key], after[key]):
            np.testing.assert_allclose(b, a, err_msg=key, **tol)
    for (ra, na, la, sa), (rb, nb, lb, sb) in zip(before["samples"], after["samples"]):
        assert list(ra) == list(rb) and np.array_equal(na, nb) and sa == sb
        np.testing.assert_allclose(lb, la, **tol)


# ---- 9. the min_prob filter

def test_min_prob_filters_on_the_larger_of_the_two():
    seqs, quals = batch((25, 80, 131), seed=21, neg_every=0)
    eng = api.Engine(P1, PAR, 50, 30, 1e-4, 0.1, 0, 0)
    eng.load_batch(seqs, quals)
    x = perturbed(eng)
    full = eng.conditional_pairs(x, 0.0)
    for m in (1e-6, 1e-3, 0.3):
        got = eng.conditional_pairs(x, m)
        n_kept = 0
        for f, g in zip(full, got):
            sel = np.maximum(f["p_motif"], f["p_none"]) >= m
            # (two runs agree to rounding: a cell within rounding of the threshold may fall on either side)
            edge = np.abs(np.maximum(f["p_motif"], f["p_none"]) - m) <= 1e-10 * m
            assert not edge.any()
            assert np.array_equal(g["i"], f["i"][sel]) and np.array_equal(g["j"], f["j"][sel])
            np.testing.assert_allclose(g["p_motif"], f["p_motif"][sel], rtol=1e-10, atol=1e-14)
            np.testing.assert_allclose(g["p_none"], f["p_none"][sel], rtol=1e-10, atol=1e-14)
            np.testing.assert_allclose(g["unpaired_none"], f["unpaired_none"], rtol=1e-10, atol=1e-14)
            assert "structure_motif" not in g
            n_kept += int(sel.sum())
        assert 0 < n_kept and (m < 0.3 or n_kept < sum(len(f["i"]) for f in full))
    # some pair is above a threshold in one fold only (and listed: the filter takes the larger of the two)
    assert any(np.any((f["p_motif"] >= m) != (f["p_none"] >= m)) for f in full for m in (1e-3, 0.3))
    for g, f in zip(eng.conditional_pairs(x, float("inf")), full):
        assert len(g["i"]) == 0 and len(g["unpaired_motif"]) == len(f["unpaired_motif"])


# ---- 10. refusals

def raw_call(eng, x, min_prob=0.0, gamma=1.0, structures=False, n_pairs=True):
    lib = api.load_library()
    dp = C.POINTER(C.c_double)
    m = C.c_int64()
    buf = C.create_string_buffer(4096) if structures else None
    return lib.elemdp_pair_conditional(eng._h, x.ctypes.data_as(dp) if x is not None else None, eng.n_param, min_prob, gamma,
                                       C.byref(m) if n_pairs else None, None, None, None, buf, None, None), m.value


def test_refusals():
    EINVAL, ESTATE = -1, -4
    lib = api.load_library()
    eng = api.Engine(P1, PAR, 50, 30, 1e-4, 0.1, 0, 0)
    x = np.zeros(eng.n_param)
    assert raw_call(eng, x)[0] == ESTATE                                   # before load_batch
    assert lib.elemdp_pair_conditional_list(eng._h, None, None, None, None, None, 0) == ESTATE
    seqs, quals = batch((20, 31), seed=1)
    eng.load_batch(seqs, quals)
    x = perturbed(eng)
    assert lib.elemdp_pair_conditional_list(eng._h, None, None, None, None, None, 1 << 20) == ESTATE      # no conditional call yet
    eng.pair_posteriors(x, 0.0)
    assert lib.elemdp_pair_conditional_list(eng._h, None, None, None, None, None, 1 << 20) == ESTATE      # (a pair call is none)
    for bad in (-1e-9, -1.0, float("nan")):
        assert raw_call(eng, x, min_prob=bad)[0] == EINVAL
    for gamma in (0.0, -1.0, float("nan"), float("inf")):
        assert raw_call(eng, x, gamma=gamma, structures=True)[0] == EINVAL
        assert raw_call(eng, x, gamma=gamma, structures=False)[0] == 0      # gamma is looked at only with a structure
    assert raw_call(eng, None)[0] == EINVAL and raw_call(eng, x, n_pairs=False)[0] == EINVAL
    i32, dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    dpx = x.ctypes.data_as(dp)
    m = C.c_int64()
    assert lib.elemdp_pair_conditional(eng._h, dpx, eng.n_param + 1, 0.0, 1.0, C.byref(m), None, None, None, None, None, None) == EINVAL
    rc, n = raw_call(eng, x)
    assert rc == 0 and n > 1
    seq = np.zeros(n, dtype=np.int32)
    assert lib.elemdp_pair_conditional_list(eng._h, seq.ctypes.data_as(i32), None, None, None, None, n - 1) == EINVAL
    assert lib.elemdp_pair_conditional_list(eng._h, seq.ctypes.data_as(i32), None, None, None, None, n) == 0
    assert seq[0] == 0 and seq[-1] == 1 and np.all(np.diff(seq) >= 0)
    assert raw_call(eng, x, min_prob=float("inf"))[1] == 0
    eng.load_batch(seqs, quals)
    assert lib.elemdp_pair_conditional_list(eng._h, None, None, None, None, None, 1 << 20) == ESTATE      # a new resident batch


# ---- 11. command line

def test_command_line_writes_the_contrast_file(tmp_path):
    fq, model = gpath("positive_head6.fq"), gpath("trna_a.model")
    a1, cf = str(tmp_path / "a.raw"), str(tmp_path / "contrast.txt")
    cli.main(["scan", "-f", fq, "-q", model, "--out1", a1, "--out-contrast", cf, "--chunk", "4", "--contrast-min-prob", "1e-2",
              "--contrast-gamma", "2.0"])
    recs = io.read_fastq(fq)
    got = io.read_contrast_records(cf)
    assert [g["id"] for g in got] == [r[0] for r in recs] and len(recs) > 4
    m = io.read_model(model)
    eng = io.engine_from_model(m)
    eng.load_batch([s for _, s, _ in recs], [q for _, _, q in recs])
    want = eng.conditional_pairs(m["x"], 1e-2, 2.0)
    # (the printed 6 digits; the tables are summed with LDS atomics, so a run differs from another in the last bits)
    tol = dict(rtol=2e-6, atol=1e-12)

    def printed(v):
        return np.array([float(io.fmt(float(u))) for u in np.atleast_1d(v)])

    for g, w in zip(got, want):
        assert (g["structure_motif"], g["structure_none"]) == (w["structure_motif"], w["structure_none"]), g["id"]
        np.testing.assert_allclose(g["exist_prob"], printed(w["exist_prob"])[0], **tol)
        np.testing.assert_allclose(g["shift"], printed(w["shift"])[0], equal_nan=True, **tol)
        np.testing.assert_allclose(g["unpaired_motif"], printed(w["unpaired_motif"]), **tol)
        np.testing.assert_allclose(g["unpaired_none"], printed(w["unpaired_none"]), **tol)
        assert [(i, j) for i, j, _, _ in g["pairs"]] == [(int(i) + 1, int(j)) for i, j in zip(w["i"], w["j"])], g["id"]
        np.testing.assert_allclose([p for _, _, p, _ in g["pairs"]], printed(w["p_motif"]), **tol)
        np.testing.assert_allclose([p for _, _, _, p in g["pairs"]], printed(w["p_none"]), **tol)
    # the reader round-trips what the writer prints
    text = "".join(io.contrast_record(g["id"], dict(g, i=np.array([p[0] - 1 for p in g["pairs"]]), j=np.array([p[1] for p in g["pairs"]]),
                                                    p_motif=[p[2] for p in g["pairs"]], p_none=[p[3] for p in g["pairs"]])) for g in got)
    assert text == open(cf).read()
