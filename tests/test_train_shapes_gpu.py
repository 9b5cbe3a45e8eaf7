"""Train evaluation against the oracle, sequence by sequence, at the shapes, groupings, kernel forms and
models where the train kernels have code of their own: sequences across the 256-lane blocks and beyond the staged exterior
chain, band widths from 20 to 300 (the LDS window of k4_in / k4_out and with it their instantiation), every option that changes
the kernels or the schedule, slot reuse, two group streams, a group too large for the exterior ring, log-space chunks, other
models, edge and skipped sequences, streamed batches, ranged evaluations, and an evaluation behind the scan family on the same
slots.  Every case goes through tests/train_check.py: check_train_path (seq_stats and the count columns ENo, ENx, EHo, EHx of
every sequence; fn, gr, sum_eff, n_skipped and the count segments of train_partial; a repeated evaluation).

Labels: every sequence appears once with the motif and once without (final quality 5), so that a fault tied to one length or one
partial workgroup shows unattenuated in one of the two (train_check's docstring).  Every case asserts how many of its sequences
the oracle did not skip, by label; test_train_shapes_cpu.py asserts the same counts from the oracle alone.

The cases A to D run with ELEMDP_LDS_DEBUG set and record what launch_lin_group says it launched;
test_every_band_kernel_form_was_launched, the last test of the file, requires every instantiation of k4_in and of
k4_out<OUT_TRAIN> and both values of stage_ext, ext_ring and ext_nt among them."""
import re

import numpy as np
import pytest

from oracle import pyoracle as po
from rnaelem_amd import api, io
from tests import train_check as tc
from tests.test_pair_posterior_gpu import perturbed
from tests.test_pair_shapes_gpu import batch, edge_batch, oracle_maker
from tests.util import gpath

pytestmark = pytest.mark.gpu

PAR = "~T2004~"
P1, P2 = "((.*.))", "(((((.*.)))))(((.*.)))"


# ---- the cases (shared with test_train_shapes_cpu.py)

A_CASES = [(P1, (255, 256, 257, 511, 512, 600)), (P1, (2300, 60)), (P2, (600, 257, 70))]
B_GRID = [(20, 5), (33, 30), (50, 0), (100, 30), (200, 30), (255, 30), (300, 30)]
C_LENS = (13, 40, 97, 131, 200, 257, 300)
C_OPTS = {
    "default": ((), 0),
    "fast0": ((("fast", 0),), 0),
    "prune0": ((("prune", 0),), 0),
    "deterministic": ((("deterministic", 1),), 0),
    "dbg8": ((("dbg", 8),), 0),
    "schedule0": ((("schedule", 0),), 0),
    "schedule0-fast0": ((("schedule", 0), ("fast", 0)), 0),
    "pipeline3": ((("pipeline", 3),), 0),
    "group_streams1": ((("group_streams", 1),), 0),
    "lik-ratio": ((), api.LIK_RATIO),
    "lik-ratio-schedule0": ((("schedule", 0),), api.LIK_RATIO),
}
C_PATTERNS = {".": 7, "(.)*(.)": 7, P2: 5, "(*(.)*)": 7}        # (the sequences of forms_batch unskipped, of 7 per label)
F_MODELS = ["syn_sm.model", "syn_a2007.model", "syn_c12.model", "tiny_a.model", "tiny_ne.model", "1.model", "2.model", "3.model"]


def long_batch(lens):
    return tc.relabelled(*batch(lens, seed=sum(lens), neg_every=0))


def longest_of(W):
    """2 W + 7, cut down at W >= 255 where the oracle's time goes with L W^2 (the width stays)"""
    return 2 * W + 7 if W <= 200 else W + 40


def width_batch(W, C):
    """lengths 1, 2, 5 (no room for the motif: skipped), W - 1, W, W + 1 and the longest; for W >= 100 also the G^h AAAA C^h
    hairpin that spans the band"""
    lens = [1, 2, 5, W - 1, W, W + 1, longest_of(W)]
    seqs, quals = batch(lens, seed=1000 * W + C, neg_every=0)
    if W >= 100:
        h = W // 2 - 2
        seqs.append(np.array([3] * h + [1, 1, 1, 1] + [2] * h, dtype=np.uint8))
        quals.append(np.full(2 * h + 5, 10, dtype=np.uint8))
    return tc.relabelled(seqs, quals)


def forms_batch():
    return tc.relabelled(*batch(C_LENS, seed=31, neg_every=0))


def three_slot_batch():
    lens = [int(v) for v in np.linspace(20, 280, 20)][::-1]
    lens[3], lens[11] = lens[11], lens[3]     # (not sorted: the processing order differs from the batch order)
    return tc.relabelled(*batch(lens, seed=5, neg_every=0))


def two_stream_batch():
    rng = np.random.default_rng(64)
    return tc.relabelled(*batch([int(v) for v in rng.integers(30, 121, size=96)], seed=64, neg_every=0))


def large_group_batch():
    rng = np.random.default_rng(1100)
    return tc.relabelled(*batch([int(v) for v in rng.integers(8, 41, size=550)], seed=1100, neg_every=0))


def log_space_batch():
    """the 8 sequences of syn_L150_n8.fq, which leave the double range at lambda = 40, between short ones that do not"""
    recs = io.read_fastq(gpath("syn_L150_n8.fq"))
    short_s, short_q = batch((4, 6, 9, 12, 16, 24), seed=40, neg_every=0)
    seqs = short_s[:3] + [s for _, s, _ in recs][:4] + short_s[3:] + [s for _, s, _ in recs][4:]
    quals = short_q[:3] + [q for _, _, q in recs][:4] + short_q[3:] + [q for _, _, q in recs][4:]
    return tc.relabelled(seqs, quals)


def model_batch(model):
    return tc.relabelled(*batch((3, 13, 40, 97, 131, 200), seed=len(model), neg_every=0))


def edge_case_batch():
    return tc.relabelled(*edge_batch())


def all_skipped_batch():
    """under `(.........)`: nothing here has room for the motif or a pair to close it"""
    enc = {"A": 1, "C": 2, "G": 3, "U": 4}
    seqs = [np.array([enc[c] for c in "GGGAAAUCCC"], dtype=np.uint8), np.zeros(30, dtype=np.uint8), np.ones(40, dtype=np.uint8),
            np.array([3], dtype=np.uint8), np.array([3, 2], dtype=np.uint8), np.array([3, 1, 1, 1, 2], dtype=np.uint8)]
    return tc.relabelled(seqs, [np.full(len(s) + 1, 10, dtype=np.uint8) for s in seqs])


def n_base_batch():
    return tc.relabelled(*batch((30, 64, 97, 150, 257), seed=14, n_every=1, neg_every=0))


def streamed_batch():
    return tc.relabelled(*batch([40 + 15 * k for k in range(20)], seed=77, neg_every=0))


def ranged_batch():
    rng = np.random.default_rng(32)
    return tc.relabelled(*batch([int(v) for v in rng.integers(20, 260, size=16)], seed=32, neg_every=0))


WINDOWS = [(0, 7), (7, 12), (19, 13), (31, 1)]


def maker(pattern, W, C, x, flags=0):
    if not flags:
        return oracle_maker(pattern, W, C, x)

    def make():
        o = po.make_oracle(pattern, W, C, min_bpp=1e-4, tau=0.1, flags=flags)
        o.set_params(x)
        return o
    return make


def assert_unskipped(refs, quals, at_least=None, exactly=None, first=0, count=None):
    """at_least: a fraction of each label's sequences; exactly: (with motif, without motif)"""
    got = refs.unskipped(quals, first, count)
    if exactly is not None:
        assert got == tuple(exactly), (got, exactly)
    else:
        n = (len(quals) if count is None else count)
        labels = [tc.has_motif(q) for q in quals[first:first + n]]
        want = (at_least * sum(labels), at_least * (n - sum(labels)))
        assert got[0] >= want[0] and got[1] >= want[1], (got, want)


# ---- the kernel forms that launch_lin_group names under ELEMDP_LDS_DEBUG

FORMS = dict(k4_in=set(), k4_out=set(), stage_ext=set(), ext_nt=set(), ext_ring=set(), n_pass=set(), combine=set())
LINE = re.compile(r"lin group: G (\d+) .* forms k4_in (\S+) k4_out (\S+) stage_ext (\d+) ext_nt (\d+) ext_ring (\d+) n_pass (\d+) combine (\d+)")


@pytest.fixture
def forms(monkeypatch, capfd):
    """sets ELEMDP_LDS_DEBUG; forms() returns what the launches since the last call were and adds it to FORMS"""
    monkeypatch.setenv("ELEMDP_LDS_DEBUG", "1")

    def read():
        seen = [m.groups()[1:] + m.groups()[:1] for m in map(LINE.search, capfd.readouterr().err.splitlines()) if m]     # (G last)
        for g in seen:
            for key, v in zip(("k4_in", "k4_out", "stage_ext", "ext_nt", "ext_ring", "n_pass", "combine"), g):
                FORMS[key].add(v)
        return seen
    return read


def run(pattern, seqs, quals, W=50, C=30, opts=(), flags=0, x=None, refs=None, rows=True, window=None, eng=None):
    if eng is None:
        eng = api.Engine(pattern, PAR, W, C, 1e-4, 0.1, flags, 0)
        for k, v in opts:
            eng.set_option(k, v)
    if window is None or eng.n_seq == 0:
        eng.load_batch(seqs, quals)
    if x is None:
        x = perturbed(eng)
    refs, res, stats, counts = tc.check_train_path(eng, seqs, quals, x, maker(pattern, W, C, x, flags), refs=refs, rows=rows,
                                                   window=window)
    return eng, x, refs, res, stats, counts


# ---- A. long sequences

@pytest.mark.parametrize("pattern,lens", A_CASES)
def test_long_sequences(pattern, lens, forms):
    """L >= 256: the exterior-chain kernels stride over the sequence in blocks, k4_out's statistics cross many workgroups per
    diagonal; L = 2300 takes the exterior-chain kernels that cannot stage the sequence in LDS (stage_ext 0); the S = 59 pattern
    has four cells per workgroup."""
    seqs, quals = long_batch(lens)
    eng, x, refs, _, _, _ = run(pattern, seqs, quals)
    assert_unskipped(refs, quals, exactly=(len(lens), len(lens)))
    seen = forms()
    assert seen and all(g[2] == ("0" if max(lens) > 2048 else "1") for g in seen), seen


# ---- B. band widths

@pytest.mark.parametrize("W,C", B_GRID)
def test_band_widths(W, C, forms):
    """W != 50: win = cpb + W + 3 sizes the LDS of k4_in / k4_out and moves them between the instantiations that ask for eight /
    six waves per SIMD and the plain ones; L <= W gives the sequence its own W = L; L = 1, 2, 5 hold no motif and are skipped
    (their count columns stay 0 among live neighbours); C = 0 and C = 5 cut the interior loops."""
    seqs, quals = width_batch(W, C)
    eng, x, refs, _, _, _ = run(P1, seqs, quals, W=W, C=C)
    n = len(seqs) // 2 - 3
    assert all(refs.seq[k]["skipped"] and refs.seq[k]["Zari"] == -np.inf for k in range(6))
    assert_unskipped(refs, quals, exactly=(n, n))
    assert forms()


# ---- C. forms

@pytest.fixture(scope="module")
def form_refs():
    seqs, quals = forms_batch()
    x = perturbed(api.Engine(P1, PAR, 50, 30, 1e-4, 0.1, 0, 0))
    refs = {fl: tc.oracle_train_refs(maker(P1, 50, 30, x, fl), seqs, quals) for fl in (0, api.LIK_RATIO)}
    return seqs, quals, x, refs


@pytest.mark.parametrize("name", list(C_OPTS))
def test_options_and_schedules(name, form_refs, forms):
    """Every option that changes the train kernels or their schedule, on one batch with the oracle's rows computed once: the
    band kernels without the tables (fast 0: the blob staged; dbg 8: not staged, the generic ones), unpruned lists, the deterministic sums (k4_combine's block order), the reference's two outside
    passes (schedule 0, without k4_combine unless LIK_RATIO), the log-space pipeline alone, one group stream, and the
    likelihood-ratio objective under both schedules (the roles of the passes swap for a sequence without the motif; the rows
    hold the reference's (o, x) all the same)."""
    seqs, quals, x, refs = form_refs
    opts, flags = C_OPTS[name]
    eng, _, _, res, stats, counts = run(P1, seqs, quals, opts=opts, flags=flags, x=x, refs=refs[flags])
    assert_unskipped(refs[flags], quals, at_least=0.9)
    seen = forms()
    if name == "pipeline3":
        assert not seen
    else:
        sched0 = dict(opts).get("schedule", 1) == 0
        assert seen and all(g[5] == ("2" if sched0 else "1") for g in seen), seen
        assert all(g[6] == ("0" if sched0 and not flags else "1") for g in seen), seen
    if name == "deterministic":         # bit for bit from one evaluation to the next
        res2 = eng.train_eval(x)
        c2 = eng.seq_counts()
        assert res2[0] == res[0] and np.array_equal(res2[1], res[1])
        assert np.array_equal(eng.seq_stats(), stats, equal_nan=True)
        assert all(np.array_equal(c2[key], counts[key]) for key in tc.COUNTS)


@pytest.mark.parametrize("pattern", list(C_PATTERNS))
def test_patterns_of_the_other_instantiations(pattern, forms):
    """`.` (S = 6, the most cells per workgroup), `(.)*(.)` and `(*(.)*)` (a pair list of three: table-driven, but not the form
    unrolled for two), the S = 59 pattern (the fewest cells per workgroup: 4)"""
    seqs, quals = forms_batch()
    _, _, refs, _, _, _ = run(pattern, seqs, quals)
    assert_unskipped(refs, quals, exactly=(C_PATTERNS[pattern],) * 2)          # (L = 13 and 40 have no room for the S = 59 pattern)
    assert forms()


# ---- D. groups

def test_three_slots_reused_by_fourteen_groups(forms):
    """group 3 on 40 unsorted sequences (20 lengths 20 .. 280 under both labels): 14 groups reuse 3 slots on one stream.  A group that reads the tables or the statistics
    of the group before it gives another sequence's rows."""
    seqs, quals = three_slot_batch()
    _, _, refs, _, _, _ = run(P1, seqs, quals, opts=(("group", 3),))
    assert_unskipped(refs, quals, at_least=0.9)
    assert len(forms()) >= 3 * 14            # (three evaluations of fourteen groups)


def test_two_group_streams_with_three_groups_each(forms):
    """192 sequences of L 30 .. 120, group 64: n >= 64 with 64 slots, so two group streams of 32 slots and ceil(192 / 32) = 6
    groups of 32: three per stream, stream 1 at slot0 = 32.  Every sequence against the oracle, so that both streams being wrong
    the same way cannot pass."""
    seqs, quals = two_stream_batch()
    _, _, refs, _, _, _ = run(P1, seqs, quals, opts=(("group", 64),))
    assert_unskipped(refs, quals, at_least=0.9)
    seen = forms()
    assert len(seen) == 3 * 6 and all(g[7] == "32" for g in seen), seen[:2]


def test_one_group_too_large_for_the_exterior_ring(forms):
    """1100 short sequences in ONE group (group 1100, one group stream): G > 1024, so group_geometry drops the LDS ring of the
    exterior-chain kernels (ext_ring 0) and their wide workgroups (ext_nt 128)."""
    seqs, quals = large_group_batch()
    _, _, refs, _, _, _ = run(P1, seqs, quals, opts=(("group", 1100), ("group_streams", 1)))
    assert_unskipped(refs, quals, at_least=0.9)
    seen = forms()
    assert seen and all(g[4] == "0" and g[3] == "128" and g[7] == "1100" for g in seen), seen[:3]


def test_a_shorter_and_smaller_batch_on_the_same_engine(forms):
    """load_batch after an evaluation of a larger batch: the slots, d_seq_out_ and the plans of the first batch stay allocated;
    nothing of it may show in the rows of the second"""
    seqs, quals = forms_batch()
    eng, x, refs, _, _, _ = run(P1, seqs, quals)
    s2, q2 = tc.relabelled(*batch((21, 55, 90), seed=9, neg_every=0))
    _, _, refs2, _, _, _ = run(P1, s2, q2, x=x, eng=eng)
    assert_unskipped(refs2, q2, exactly=(3, 3))
    assert eng.seq_counts()["ENo"].shape[0] == 6
    assert forms()


# ---- E. log space

def test_flagged_sequences_in_several_log_space_chunks():
    """lambda = 40: the L = 150 sequences leave the double range of the scaled-linear tables and are re-evaluated by the
    log-space pipeline in chunks of n_dense <= n_slots = 2 (option group 2) -- their rows are written by k3_combine and match the
    oracle like any other -- while the short ones stay on the scaled-linear path."""
    seqs, quals = log_space_batch()
    x = api.Engine(P1, PAR, 50, 30, 1e-4, 0.1, 0, 0).initial_params(40.0)
    eng, _, refs, _, _, _ = run(P1, seqs, quals, opts=(("group", 2),), x=x)
    n_flagged = int(eng.last_timing()[2])
    assert 2 * 2 < n_flagged < len(seqs), n_flagged          # (at least three chunks of at most 2)
    assert refs.unskipped(quals)[0] >= 8 and refs.unskipped(quals)[1] >= 8


def test_log_space_pipeline_over_several_groups():
    """pipeline 3, group 4: every sequence through the log-space pipeline, 14 sequences in groups of at most 4"""
    seqs, quals = forms_batch()
    _, _, refs, _, _, _ = run(P1, seqs, quals, opts=(("pipeline", 3), ("group", 4)))
    assert_unskipped(refs, quals, at_least=0.9)


# ---- F. models

@pytest.mark.parametrize("model", F_MODELS)
def test_models(model):
    """Through io.engine_from_model / po.oracle_from_model: softmax theta (syn_sm, 1: gr goes through the chain rule of
    train_finish, the counts do not), ~A2007~, W 40 / C 12, W 30, no energy (tiny_ne), W 20 / C 999 (1), --no-rss (2: no band
    sweeps at all) and 3."""
    m = io.read_model(gpath(model))
    seqs, quals = model_batch(model)
    eng = io.engine_from_model(m)
    eng.load_batch(seqs, quals)
    x = m["x"]
    _, xo = po.oracle_from_model(gpath(model))
    np.testing.assert_array_equal(x, xo)
    refs, res, _, _ = tc.check_train_path(eng, seqs, quals, x, lambda: po.oracle_from_model(gpath(model))[0])
    got = refs.unskipped(quals)
    assert got[0] == got[1] >= 4, got


# ---- G. edge sequences

@pytest.mark.parametrize("pattern", ["(.........)", P1])
def test_edge_sequences(pattern):
    """GGGAAAUCCC, all N, poly-A, L = 1 and L = 2 between live sequences of one group: the skipped ones keep count columns of
    exactly 0 (k_reduce sums every row), no NaN from 1 / Z, and their neighbours stay exact."""
    seqs, quals = edge_case_batch()
    _, _, refs, res, _, _ = run(pattern, seqs, quals)
    live = [k for k in range(len(seqs)) if not refs.seq[k]["skipped"]]
    hairpin = [] if pattern == "(.........)" else [2, 3]
    assert live == sorted([0, 1, 6, 7, 12, 13] + hairpin), live      # (exactly the edge entries are skipped)
    assert res[3] == len(seqs) - len(live)


def test_a_batch_the_oracle_skips_entirely():
    seqs, quals = all_skipped_batch()
    eng, x, refs, res, stats, counts = run("(.........)", seqs, quals)
    assert_unskipped(refs, quals, exactly=(0, 0))
    fn, gr, eff, nsk = res
    assert fn == 0.0 and np.all(gr == 0.0) and nsk == len(seqs) and eff == 0.0
    assert all(np.all(counts[key] == 0.0) for key in tc.COUNTS)
    assert np.all(eng.train_partial(x)[4:] == 0.0)


def test_n_bases_in_every_sequence():
    seqs, quals = n_base_batch()
    assert all((s == 0).any() for s in seqs)
    _, _, refs, _, _, _ = run(P1, seqs, quals)
    assert_unskipped(refs, quals, exactly=(5, 5))


# ---- H. streamed

def test_streamed_batch_against_the_oracle():
    """max_resident 7: chunks of 7 sequences on inner engines; seq_stats per sequence and the count sums of train_partial against
    the oracle; the per-sequence counts are not kept and seq_counts says so"""
    seqs, quals = streamed_batch()
    eng = api.Engine(P1, PAR, 50, 30, 1e-4, 0.1, 0, 0)
    eng.set_option("max_resident", 7)
    eng.load_batch(seqs, quals)
    x = perturbed(eng)
    with pytest.raises(api.ElemdpError) as e:
        eng.seq_counts()
    assert e.value.code == -4
    refs, _, _, counts = tc.check_train_path(eng, seqs, quals, x, maker(P1, 50, 30, x), rows=False)
    assert counts is None
    assert_unskipped(refs, quals, at_least=0.9)
    with pytest.raises(api.ElemdpError) as e:
        eng.seq_counts()
    assert e.value.code == -4                                          # ELEMDP_ESTATE


def test_seq_counts_call_order():
    """ESTATE before load_batch, before the first evaluation of a batch and behind a scan (whose rows are not the train's)"""
    seqs, quals = tc.relabelled(*batch((30, 60), seed=2, neg_every=0))
    eng = api.Engine(P1, PAR, 50, 30, 1e-4, 0.1, 0, 0)
    x = perturbed(eng)

    def refused():
        with pytest.raises(api.ElemdpError) as e:
            eng.seq_counts()
        return e.value.code == -4
    assert refused()
    eng.load_batch(seqs, quals)
    assert refused()
    eng.train_eval(x)
    assert eng.seq_counts()["ENo"].shape == (4, eng.n_param - 2)
    eng.scan(x)
    assert refused()
    eng.train_partial(x)
    assert eng.seq_counts()["EHx"].shape == (4, 2)
    eng.load_batch(seqs[:2], quals[:2])
    assert refused()


# ---- I. ranged evaluation

def test_ranged_evaluations_against_the_oracle():
    """eval_first / eval_count on a resident batch of 32 ragged sequences: each window's rows and sums against the oracle for that
    window (not only against a reloaded engine), on one engine, one window after the other"""
    seqs, quals = ranged_batch()
    eng = api.Engine(P1, PAR, 50, 30, 1e-4, 0.1, 0, 0)
    eng.load_batch(seqs, quals)
    x = perturbed(eng)
    refs = tc.oracle_train_refs(maker(P1, 50, 30, x), seqs, quals)
    assert_unskipped(refs, quals, at_least=0.9)
    for w in WINDOWS:
        tc.check_train_path(eng, seqs, quals, x, maker(P1, 50, 30, x), refs=refs, window=w)
    tc.check_train_path(eng, seqs, quals, x, maker(P1, 50, 30, x), refs=refs)          # (and the whole batch behind them)


# ---- J. after the scan family

def test_train_eval_after_the_scan_family():
    """scan, pair_posteriors and sample_structures leave dense / trace tables and rows of their own over the same slots; the next
    train evaluation still matches the oracle"""
    seqs, quals = forms_batch()
    eng = api.Engine(P1, PAR, 50, 30, 1e-4, 0.1, 0, 0)
    eng.load_batch(seqs, quals)
    x = perturbed(eng)
    refs = tc.oracle_train_refs(maker(P1, 50, 30, x), seqs, quals)
    for call in (lambda: eng.scan(x), lambda: eng.pair_posteriors(x, 0.0), lambda: eng.sample_structures(x, 3, seed=1)):
        call()
        tc.check_train_path(eng, seqs, quals, x, maker(P1, 50, 30, x), refs=refs)


# ---- the forms the cases A to D went through (last: it reads what they recorded)

K4_FORMS = {"fp2-waves", "fp2", "fast", "staged", "generic"}


def test_every_band_kernel_form_was_launched():
    """launch_k4_in and launch_k4_out<OUT_TRAIN> have five branches each; every one, and both values of stage_ext, ext_ring and
    ext_nt, must have been taken by the cases above (run the whole file: this test reads what they recorded)."""
    print("band-kernel instantiations launched: k4_in %s; k4_out %s; stage_ext %s; ext_nt %s; ext_ring %s; n_pass %s; combine %s" % tuple(
        sorted(FORMS[k]) for k in ("k4_in", "k4_out", "stage_ext", "ext_nt", "ext_ring", "n_pass", "combine")))
    print("worst per-sequence count error |gpu - oracle| / (%g + |oracle|) = %.3e at %s" % (
        tc.ROW_ATOL / tc.ROW_RTOL, tc.WORST["err"], tc.WORST["where"]))
    assert FORMS["k4_in"] == K4_FORMS, FORMS["k4_in"]
    assert FORMS["k4_out"] == K4_FORMS, FORMS["k4_out"]
    assert FORMS["stage_ext"] == {"0", "1"} and FORMS["ext_ring"] == {"0", "1"} and len(FORMS["ext_nt"]) == 2, FORMS
    assert FORMS["n_pass"] == {"1", "2"} and FORMS["combine"] == {"0", "1"}, FORMS
