"""Samples of derivations at the shapes, groupings, forms and models where the sampler has addressing and
scheduling of its own: walk stacks per slot and lane with one cap per ragged group, int16 frames at L = 2300, the output layout
n_samples * seq_base + k * L, the lane rounds of k_sample (64) and of k_dp (256), several groups per stream and two group
streams, both forms in one call, log-space chunks, other models, edge sequences, streamed batches.  Every case goes through
tests/sample_check.py: check_sample_path -- status, validity, the same draws as the CPU driver (>= 99.9 %), the exact
log-probability of picked samples against the oracle's weight of that one derivation, and in the cases marked (e) the
frequencies against the oracle's posteriors.  The seeds of the (e) cases were kept after the CPU driver's samples of the same
case passed the same frequency check, so that a failure on the GPU is the kernel's; the log-space form has no CPU driver, so
the seed of the flagged sequences of case E1 could not be tried that way."""
import numpy as np
import pytest

from oracle import pyoracle as po
from rnaelem_amd import api, io
from tests.pair_check import oracle_refs
from tests.sample_check import Driver, check_sample_path, distinct, driver_from_model
from tests.test_pair_posterior_gpu import perturbed
from tests.test_pair_shapes_gpu import C_LENS, C_OPTS, P1, P2, PAR, batch, edge_batch, oracle_maker
from tests.util import gpath

pytestmark = pytest.mark.gpu

N_SAMPLES = 130     # two full lane rounds of k_sample and a partial one
N_DIST = 4000       # the (e) cases


def make_engine(pattern, W=50, C=30, opts=()):
    eng = api.Engine(pattern, PAR, W, C, 1e-4, 0.1, 0, 0)
    for k, v in opts:
        eng.set_option(k, v)
    return eng


def run(pattern, seqs, quals, W=50, C=30, opts=(), x=None, n_samples=N_SAMPLES, seed=1, fast=True, engine=make_engine, **kw):
    eng = engine(pattern, W, C, opts)
    eng.load_batch(seqs, quals)
    if x is None:
        x = perturbed(eng)
    drv = Driver(pattern, PAR, W, C)
    drv.set_fast(fast)
    out = check_sample_path(eng, seqs, quals, x, oracle_maker(pattern, W, C, x), n_samples, seed, drv=drv, **kw)
    return eng, x, out


def single_derivation(out, k):
    rss, nodes, logp, st = out["res"][k]
    assert st == 0 and len(distinct(rss, nodes)) == 1 and np.all(np.abs(logp) <= 1e-12), (k, logp[:3])


# ---- A. long sequences

A_CASES = [(P1, (255, 256, 257, 511, 512, 600)), (P1, (2300, 60)), (P2, (600, 257, 70))]


@pytest.mark.parametrize("pattern,lens", A_CASES)
def test_long_sequences(pattern, lens):
    """One group: every slot's stacks are 64 x (Lmax + 4) frames, so a short neighbour of a long sequence walks on a stack
    addressed with the long one's cap; TraceFrame and SampleStep hold positions up to 2300 in int16; L = 2300 takes the
    exterior chain that cannot stage the sequence in LDS."""
    seqs, quals = batch(lens, seed=sum(lens))
    _, _, out = run(pattern, seqs, quals, what="A %s %s" % (pattern, lens))
    assert all(st == 0 for _, _, _, st in out["res"])
    k = int(np.argmax(lens))
    assert any("R" in r[256:] for r in out["res"][k][0]), "no sampled pair beyond base 256"


# ---- B. band widths

B_CASES = [(20, 5), (33, 30), (100, 30), (200, 30), (255, 30), (300, 30)]


def b_batch(W, C):
    seqs, quals = batch([1, 2, 5, W - 1, W, W + 1, 2 * W + 7], seed=1000 * W + C)
    if W >= 100:
        h = W // 2 - 2
        seqs.append(np.array([3] * h + [1, 1, 1, 1] + [2] * h, dtype=np.uint8))
        quals.append(np.full(2 * h + 5, 10, dtype=np.uint8))
        quals[-1][-1] = 0
    return seqs, quals


@pytest.mark.parametrize("W,C", B_CASES)
def test_band_widths(W, C):
    """Rows of W + 1, i0 = j - W in rule 7, a sequence's own W = L for L <= W; L = 1, 2, and L = 5 unless its ends pair and the
    filter keeps that cell, hold one derivation (every sample identical, logp = 0); for W >= 100 the G^h AAAA C^h hairpin is the deepest nesting a walk meets; above W = 200 the BPP
    filter runs in log space."""
    seqs, quals = b_batch(W, C)
    eng, _, out = run(P1, seqs, quals, W=W, C=C, what="B W %d C %d" % (W, C))
    for k in range(3):
        if eng.pairs(k)[0].sum() == 0:
            single_derivation(out, k)
    assert eng.pairs(0)[0].sum() == 0 and eng.pairs(1)[0].sum() == 0
    if W >= 100:
        assert max(r.count("L") for r in out["res"][-1][0]) >= 10


# ---- C. layouts and kernel forms, (e)

C_SEED = 31


def c_case():
    seqs, quals = batch(C_LENS, seed=31)
    x = perturbed(api.Engine(P1, PAR, 50, 30, 1e-4, 0.1, 0, 0))
    return seqs, quals, x


@pytest.fixture(scope="module")
def layout_refs():
    seqs, quals, x = c_case()
    return seqs, quals, x, oracle_refs(oracle_maker(P1, 50, 30, x), seqs, quals)


@pytest.mark.parametrize("name", list(C_OPTS))
def test_layouts_and_kernel_forms(name, layout_refs):
    """fast 0: the generic unary phases store plane B, the table-driven ones do not (sample_bif sums it again); prune 0: complete
    lists and another column order; deterministic: another sum order.  N = 4000 with the frequencies against the oracle."""
    seqs, quals, x, refs = layout_refs
    run(P1, seqs, quals, opts=C_OPTS[name], x=x, refs=refs, n_samples=N_DIST, seed=C_SEED, fast=(name != "fast0"),
        what="C %s" % name)


# ---- D. groups and slot reuse

def test_three_slots_reused_by_seven_groups():
    """group 3, 20 sequences, one stream: 7 groups on the same three slots and the same stacks; k_sample has to run behind its
    own group's sweeps and before the next group overwrites the tables"""
    lens = [int(v) for v in np.linspace(20, 280, 20)][::-1]
    lens[3], lens[11] = lens[11], lens[3]
    seqs, quals = batch(lens, seed=5)
    run(P1, seqs, quals, opts=(("group", 3),), what="D1 group 3")


def test_two_group_streams_with_three_groups_each():
    """320 sequences, group 128: two group streams of 64 slots; the second stream's stacks start at slot0 = 64"""
    rng = np.random.default_rng(128)
    lens = [int(v) for v in rng.integers(30, 121, size=320)]
    seqs, quals = batch(lens, seed=128)
    run(P1, seqs, quals, opts=(("group", 128),), what="D2 group 128")


# ---- E. log-space form

def e1_case():
    recs = io.read_fastq(gpath("syn_L150_n8.fq"))
    short_s, short_q = batch((4, 6, 9, 12, 16, 24), seed=40, neg_every=0)
    seqs = short_s[:3] + [s for _, s, _ in recs][:4] + short_s[3:] + [s for _, s, _ in recs][4:]
    quals = short_q[:3] + [q for _, _, q in recs][:4] + short_q[3:] + [q for _, _, q in recs][4:]
    x = api.Engine(P1, PAR, 50, 30, 1e-4, 0.1, 0, 0).initial_params(40.0)
    return seqs, quals, x


def test_both_forms_in_one_call_and_several_log_space_chunks():
    """lambda = 40: the long sequences leave the double range and are sampled by k_dp<DP_SCAN> in chunks of 2 (group 2), on the
    stack buffer allocated a second time, 256 lanes per sequence (n_samples 300: two lane rounds), the short ones by k_sample
    in the same call.  The flagged ones have no CPU driver: their log-probabilities against the oracle and (e) carry them."""
    seqs, quals, x = e1_case()
    refs = oracle_refs(oracle_maker(P1, 50, 30, x), seqs, quals)
    eng, _, out = run(P1, seqs, quals, opts=(("group", 2),), x=x, n_samples=300, seed=2, refs=refs, dist="log", what="E1 lambda 40")
    n_flagged = eng.last_timing()[2]
    assert 6 <= n_flagged < len(seqs), n_flagged
    assert out["n_log"] == n_flagged


def test_log_space_pipeline_in_two_chunks():
    """pipeline 3: 1100 short sequences in chunks of 1024 and 76; stack_lanes = 20 < 256"""
    rng = np.random.default_rng(3)
    lens = [int(v) for v in rng.integers(8, 41, size=1100)]
    seqs, quals = batch(lens, seed=3)
    _, _, out = run(P1, seqs, quals, opts=(("pipeline", 3),), n_samples=20, log_all=True, what="E2 pipeline 3")
    assert sum(st == 0 for _, _, _, st in out["res"][1024:]) == 76


# ---- F. models, (e)

F_MODELS = ["syn_sm.model", "syn_a2007.model", "syn_c12.model", "tiny_a.model", "1.model", "2.model"]
F_SEED = 23


def f_case(model):
    m = io.read_model(gpath(model))
    seqs, quals = batch((3, 13, 40, 97, 131, 200), seed=len(model))
    return m, seqs, quals


@pytest.mark.parametrize("model", F_MODELS)
def test_models(model):
    """softmax theta (syn_sm, 1), ~A2007~, W 40 / C 12, W 30, W 20 / C 999, and --no-rss (2.model): no cell is kept, every
    structure is all O (rule 8 alone, as the CPU driver and the oracle's scan have it) and only the alignment varies.
    The posteriors of (e) come from the oracle with OUT_INSIDE_LOOPS: where max_iloop binds (syn_c12: C = 12 at W = 40) the
    reference's outside sweep visits interior loops that its inside sweep, and so Z, does not hold, and the posteriors formed
    from it belong to no distribution (P = 1.0086 for one pair of the L = 40 sequence, against 0.9869 with the inside's loops
    and 0.986 in the samples); for the other five models the flag changes no bit."""
    m, seqs, quals = f_case(model)
    eng = io.engine_from_model(m)
    eng.load_batch(seqs, quals)

    def make():
        return po.oracle_from_model(gpath(model))[0]

    refs = oracle_refs(lambda: po.oracle_from_model(gpath(model), extra_flags=po.OUT_INSIDE_LOOPS)[0], seqs, quals)
    if m["no_rss"]:       # (the oracle's plane P is no pair posterior there: no pair is ever drawn)
        for r in refs:
            r["P"] = np.zeros_like(r["P"])
    out = check_sample_path(eng, seqs, quals, m["x"], make, N_DIST, F_SEED, drv=driver_from_model(m), refs=refs,
                            what="F %s" % model)
    if m["no_rss"]:
        for (rss, nodes, logp, st), s in zip(out["res"], seqs):
            assert all(r == "O" * len(s) for r in rss)
        assert len(distinct(*out["res"][-1][:2])) > 10


# ---- G. edge sequences

@pytest.mark.parametrize("pattern", ["(.........)", P1])
def test_edge_sequences(pattern):
    """GGGAAAUCCC (no room for `(.........)`), all N, poly-A, L = 1 and 2 between live sequences of one group: the sequences
    without a kept pair have one derivation, every base exterior and before the motif, logp = 0"""
    seqs, quals = edge_batch()
    eng, _, out = run(pattern, seqs, quals, what="G %s" % pattern)
    for k in (2, 4, 5, 7):
        assert eng.pairs(k)[0].sum() == 0
        single_derivation(out, k)
    assert all(len(distinct(*out["res"][k][:2])) > 10 for k in (0, 3, 6))


# ---- H. streamed batch

def test_streamed_batch_with_an_index_base():
    """max_resident 7: stream_samples runs chunks of 7 on inner engines and passes index_base + the chunk's first index; the
    driver draws sequence k with index 1000 + k"""
    lens = [40 + 15 * k for k in range(20)]
    seqs, quals = batch(lens, seed=77)
    resident = make_engine(P1)
    resident.load_batch(seqs, quals)
    run(P1, seqs, quals, opts=(("max_resident", 7),), index_base=1000, mask_eng=resident, count_flagged=False, what="H streamed")


# ---- I. the output layout over n_samples

def test_sample_k_is_the_same_derivation_at_every_number_of_samples():
    """n_samples 1, 2, 63, 64, 65, 128, 129: the outputs lie at n_samples * seq_base + k * L and the stacks of min(n, 64) lanes;
    sample k is a function of (seed, index, k) alone"""
    seqs, quals = batch((13, 97, 257), seed=9)
    outs = {}
    for n in (1, 2, 63, 64, 65, 128, 129):
        outs[n] = run(P1, seqs, quals, n_samples=n, seed=4, what="I n_samples %d" % n)[2]["res"]
    top = outs[129]
    same = total = 0
    for n, res in outs.items():
        for (rss, nodes, logp, st), (rss9, nodes9, logp9, _) in zip(res, top):
            for t in range(n):
                total += 1
                same += rss[t] == rss9[t] and np.array_equal(nodes[t], nodes9[t])
    assert same >= 0.999 * total, (same, total)
