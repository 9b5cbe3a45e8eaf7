"""Pair posteriors and MEA structures (DESIGN.md sections 12 and 13) against the oracle at the shapes, layouts, groupings and
models where the pair kernels have code of their own: sequences across the 256-row blocks of k_pair_seq and k_pair_mea, band
widths from 20 to 300, the table layouts k4_pairs addresses, several groups per stream and two group streams, log-space chunks,
other models, sequences without a parse or a kept pair, streamed batches.  Every case goes through tests/pair_check.py:
check_pair_path (pair list, P, unpaired against the oracle; MEA bit for bit against the mirror and at the optimum over the
oracle's P; a sequence without the motif still has the pairs of its parses without it, from the oracle's first outside pass)."""
import numpy as np
import pytest

from oracle import pyoracle as po
from rnaelem_amd import api, io, synth
from tests.pair_check import GAMMAS, check_pair_lists, check_pair_path, oracle_refs
from tests.test_pair_posterior_gpu import perturbed
from tests.util import gpath

pytestmark = pytest.mark.gpu

PAR = "~T2004~"
P1, P2 = "((.*.))", "(((((.*.)))))(((.*.)))"


def batch(lens, seed, n_every=3, neg_every=2):
    """one synthetic sequence per length; N bases in every n_every-th sequence (L > 8), a final quality of 5 (no motif) on
    every neg_every-th one"""
    rng = np.random.default_rng(seed)
    seqs, quals = [], []
    for k, L in enumerate(lens):
        (s,), (q,) = synth.synth_batch(1, L, seed=int(rng.integers(1 << 30)))
        if n_every and k % n_every == 0 and L > 8:
            s = s.copy()
            s[rng.integers(0, L, size=max(1, L // 15))] = 0
        if neg_every and k % neg_every == 1:
            q[-1] = 5
        seqs.append(s)
        quals.append(q)
    return seqs, quals


def oracle_maker(pattern, W, C, x):
    def make():
        o = po.make_oracle(pattern, W, C, min_bpp=1e-4, tau=0.1)
        o.set_params(x)
        return o
    return make


def run(pattern, seqs, quals, W=50, C=30, opts=(), x=None, refs=None, scan=False, gammas=GAMMAS):
    eng = api.Engine(pattern, PAR, W, C, 1e-4, 0.1, 0, 0)
    for k, v in opts:
        eng.set_option(k, v)
    eng.load_batch(seqs, quals)
    if x is None:
        x = perturbed(eng)
    refs, res, mea = check_pair_path(eng, seqs, quals, x, oracle_maker(pattern, W, C, x), gammas=gammas, scan=scan, refs=refs)
    return eng, x, refs, res, mea


# ---- A. long sequences

@pytest.mark.parametrize("pattern,lens", [
    (P1, (255, 256, 257, 511, 512, 600)),
    (P1, (2300, 60)),
    (P2, (600, 257, 70)),
])
def test_long_sequences(pattern, lens):
    """L >= 256: k_pair_seq compacts the rows i = 0 .. L in blocks of 256 lanes and carries the list offset `base` from one
    block to the next; k_pair_mea's band diagonals and the unpaired loop stride over 256 lanes; L = 2300 also takes the
    exterior-chain kernels that cannot stage the sequence in LDS.  A dropped or repeated block, or a `base` carried wrong, shows
    in the list order against the kept cells, in P / unpaired beyond row 255 and in the MEA structures there."""
    seqs, quals = batch(lens, seed=sum(lens))
    eng, x, refs, res, mea = run(pattern, seqs, quals, scan=True)
    for k, L in enumerate(lens):
        if L > 256:
            assert refs[k]["P"] is not None, k
        if L >= 300:
            ii = res[k][0]
            assert len(ii) and ii.max() >= 256, k                    # (pairs in the second row block and beyond)
    assert any("(" in s[256:] for s in mea[4.0][0]), "no MEA pair beyond base 256"


# ---- B. band widths

@pytest.mark.parametrize("W,C", [(20, 5), (33, 30), (100, 30), (200, 30), (255, 30), (300, 30)])
def test_band_widths(W, C):
    """W != 50: the P / M scratch rows of W+1 and pcells = (Lmax+1)(Wmax+1); k_pair_mea's LDS window of W+1 values and its
    traceback stack of W/2+2 entries; the BPP filter in log space above W = 200.  L <= W gives the sequence its own W = L (rows
    of L+1), L = 1, 2, 5 hold no motif (only the pairs of parses without it).  For W >= 100 the G^h AAAA C^h hairpin spans the whole band: the
    deepest nesting the traceback stack has to hold.  Scan records against the oracle's too (W outside 20 .. 50)."""
    lens = [1, 2, 5, W - 1, W, W + 1, 2 * W + 7]
    seqs, quals = batch(lens, seed=1000 * W + C)
    if W >= 100:
        h = W // 2 - 2
        seqs.append(np.array([3] * h + [1, 1, 1, 1] + [2] * h, dtype=np.uint8))
        quals.append(np.full(2 * h + 5, 10, dtype=np.uint8))
        quals[-1][-1] = 0
    assert sum(len(s) > W for s in seqs) <= 2
    eng, x, refs, res, mea = run(P1, seqs, quals, W=W, C=C, scan=True)
    assert all(refs[k]["scan"]["exist_prob"] == 0.0 for k in range(3))          # (no room for the motif)
    assert sum(r["scan"]["exist_prob"] > 0.0 for r in refs) >= 3
    if W >= 100:
        depth = mea[1e3][0][-1].count("(")
        assert depth >= 10, depth                                     # (the hairpin folds into a long stem)


# ---- C. layouts and kernel forms

C_LENS = (13, 40, 97, 131, 200, 257, 300)
C_OPTS = {
    "default": (),
    "fast0": (("fast", 0),),
    "prune0": (("prune", 0),),
    "deterministic": (("deterministic", 1),),
}


@pytest.fixture(scope="module")
def layout_refs():
    seqs, quals = batch(C_LENS, seed=31)
    eng = api.Engine(P1, PAR, 50, 30, 1e-4, 0.1, 0, 0)
    x = perturbed(eng)
    return seqs, quals, x, oracle_refs(oracle_maker(P1, 50, 30, x), seqs, quals)


@pytest.mark.parametrize("name", list(C_OPTS))
def test_layouts_and_kernel_forms(name, layout_refs):
    """k4_pairs builds the row address of a cell from p_cs / p_rs, and pair_posteriors requires the P plane's columns in state
    order; fast 0 and prune 0 change the band kernels that fill the tables k4_pairs reads and prune 0 the columns, deterministic
    their sum order.  Each option set on a fresh engine against the oracle directly (a wrong row stride or column reads another
    plane's values); the default layout with the scan as well."""
    seqs, quals, x, refs = layout_refs
    run(P1, seqs, quals, opts=C_OPTS[name], x=x, refs=refs, scan=(name == "default"))


# ---- D. groups and slot reuse

def test_three_slots_reused_by_seven_groups():
    """Option group = 3 on a fresh engine: three table slots, 20 sequences, one stream (n < 128): sweep_groups gives
    ceil(20 / 3) = 7 groups of 3 (the last 2) that reuse the same slots and the same P / M scratch at slot0 = 0.  A group that
    reads the P or M scratch of the group before it, or k_pair_seq / k_pair_mea queued behind the wrong group, gives another
    sequence's values."""
    lens = [int(v) for v in np.linspace(20, 280, 20)][::-1]
    lens[3], lens[11] = lens[11], lens[3]     # (not sorted: the processing order differs from the batch order)
    seqs, quals = batch(lens, seed=5)
    eng, x, refs, _, _ = run(P1, seqs, quals, opts=(("group", 3),))
    assert sum(r["P"] is not None for r in refs) >= 15


def test_two_group_streams_with_three_groups_each():
    """320 short sequences (L = 30 .. 120), option group = 128: 128 slots, and n >= 128, so two group streams of 64 slots.
    sweep_groups: ceil(320 / 64) = 5 groups, rounded up to 6 for two streams, of ceil(320 / 6) = 54 sequences (the last 50):
    3 groups per stream, stream 1 at slot0 = 64.  k4_pairs dispatches on both streams, k_pair_mea once per group.  Every
    sequence against the oracle, so that both streams being wrong the same way cannot pass."""
    rng = np.random.default_rng(128)
    lens = [int(v) for v in rng.integers(30, 121, size=320)]
    seqs, quals = batch(lens, seed=128)
    eng, x, refs, _, _ = run(P1, seqs, quals, opts=(("group", 128),), gammas=(1e-3, 1.0, 4.0))
    assert sum(r["P"] is not None for r in refs) >= 300


# ---- E. log-space chunks

def test_flagged_sequences_in_several_log_space_chunks():
    """lambda = 40 on short sequences mixed with the 8 sequences of syn_L150_n8.fq: the long ones leave the double range of the
    scaled-linear tables and run through the fused scan kernel's first pass (the pair_p branch) in chunks of
    min(n_flagged, n_slots) = 2 sequences (option group = 2), the short ones stay on the scaled-linear path: both forms in one
    call, one list."""
    recs = io.read_fastq(gpath("syn_L150_n8.fq"))
    short_s, short_q = batch((4, 6, 9, 12, 16, 24), seed=40, neg_every=0)
    seqs = short_s[:3] + [s for _, s, _ in recs][:4] + short_s[3:] + [s for _, s, _ in recs][4:]
    quals = short_q[:3] + [q for _, _, q in recs][:4] + short_q[3:] + [q for _, _, q in recs][4:]
    x = api.Engine(P1, PAR, 50, 30, 1e-4, 0.1, 0, 0).initial_params(40.0)
    eng, _, refs, _, _ = run(P1, seqs, quals, opts=(("group", 2),), x=x)
    n_flagged = eng.last_timing()[2]          # (of the last call, mea_structures at gamma = 1e3)
    assert 6 <= n_flagged < len(seqs), n_flagged          # (>= 3 chunks of 2)
    assert sum(r["P"] is not None for r in refs) >= 8


def test_log_space_pipeline_in_two_chunks():
    """pipeline 3: every sequence in the log-space form, in chunks of max(n_blocks, 1024) sequences: 1100 short sequences
    take a chunk of 1024 and one of 76 on the same P / M scratch."""
    rng = np.random.default_rng(3)
    lens = [int(v) for v in rng.integers(8, 41, size=1100)]
    seqs, quals = batch(lens, seed=3)
    _, _, refs, res, _ = run(P1, seqs, quals, opts=(("pipeline", 3),), gammas=(1.0, 4.0))
    assert sum(r["P"] is not None for r in refs[1024:]) >= 20 and sum(len(r[2]) for r in res[1024:]) > 0


LDS_LIMIT = 160 * 1024
K_THREADS = 256          # kernels.h: kThreads


def lds_image_bytes(L, n_theta, n_small, W=50):
    """Engine::lds_layout(lay, Lmax, nword_max, scan = true), the LDS image of k_dp<DP_SCAN>, every field rounded up to 16 bytes:
    theta, en_o, en_x (8 (n_theta + 1) each), eh (8 * 4), zs (8 * 8), ws (8 (Lmax + 1)), post (8 * 3 (Lmax + 1)), the small part
    of the automaton blob (4 n_small), wave_scr (8 * 128 * kThreads / 64), the pair mask (4 nword_max, one bit per cell of
    (Lmax + 1) (W + 1): Engine::check_batch), dmin (2 (Lmax + 1)), seq and unp (Lmax + 1 each)"""
    def take(b):
        return (b + 15) & ~15
    nword = ((L + 1) * (min(L, W) + 1) + 31) // 32
    return (3 * take(8 * (n_theta + 1)) + take(8 * 4) + take(8 * 8) + take(8 * (L + 1)) + take(8 * 3 * (L + 1)) + take(4 * n_small) +
            take(8 * 128 * (K_THREADS // 64)) + take(4 * nword) + take(2 * (L + 1)) + 2 * take(L + 1))


def first_refused_length(n_theta, n_small):
    L = 1
    while lds_image_bytes(L, n_theta, n_small) <= LDS_LIMIT:
        L += 1
    return L


def test_a_sequence_beyond_the_lds_staging_is_refused_and_the_handle_lives_on():
    """The log-space form stages a sequence's rows in LDS and Engine::lds_layout refuses an image above 160 KiB; log_scan_args
    sizes it by the batch's longest sequence.  For ((.*.)) at W = 50 (n_theta 24, n_small 889 ints) the first refused length is
    3667 (163 856 bytes; L = 3666 fills the 163 840 exactly).  describe() reports n_ints, the whole blob, not its small part:
    with 0 <= n_small <= n_ints the limit lies between first_refused_length(n_theta, n_ints) and first_refused_length(n_theta,
    0) = 3752, and the batch here holds one sequence of the latter length, refused whatever the small part is, behind three
    short ones.  Under pipeline 3 scan, pair_posteriors and context_profiles throw on the host before any launch.
    The handle stays usable: under pipeline 4 the same batch gives the oracle's pair posteriors on the three short sequences
    (the long one needs no reference, it only has to be resident and swept), and a fresh batch of the three short ones under
    pipeline 3 passes the whole check."""
    eng = api.Engine(P1, PAR, 50, 30, 1e-4, 0.1, 0, 0)
    n_theta, n_ints = eng.n_param - 2, eng.describe()["layout"]["n_ints"]
    lo, L = first_refused_length(n_theta, n_ints), first_refused_length(n_theta, 0)
    assert (n_theta, L) == (24, 3752) and lo <= first_refused_length(n_theta, 889) == 3667 <= L
    assert lds_image_bytes(3666, n_theta, 889) == LDS_LIMIT
    short_s, short_q = batch((40, 71, 97), seed=160)
    (long_s,), (long_q,) = batch((L,), seed=161, n_every=0, neg_every=0)
    seqs, quals = short_s + [long_s], short_q + [long_q]
    x = perturbed(eng)
    make = oracle_maker(P1, 50, 30, x)
    refs = oracle_refs(make, short_s, short_q)
    assert sum(r["P"] is not None for r in refs) == 3
    eng.set_option("pipeline", 3)
    eng.load_batch(seqs, quals)
    for call in (lambda: eng.scan(x), lambda: eng.pair_posteriors(x, 0.0), lambda: eng.context_profiles(x)):
        with pytest.raises(api.ElemdpError, match="too large for the LDS staging"):
            call()
    eng.set_option("pipeline", 4)
    res = eng.pair_posteriors(x, 0.0)
    assert eng.last_timing()[2] == 0 and len(res) == 4 and len(res[3][3]) == L
    check_pair_lists(eng, short_s, res[:3], [r["P"] for r in refs])
    eng.set_option("pipeline", 3)
    eng.load_batch(short_s, short_q)
    check_pair_path(eng, short_s, short_q, x, make, refs=refs)
    assert eng.last_timing()[2] == 0


# ---- F. models

@pytest.mark.parametrize("model", ["syn_sm.model", "syn_a2007.model", "syn_c12.model", "tiny_a.model", "1.model", "2.model"])
def test_models(model):
    """Through io.engine_from_model / po.oracle_from_model: softmax theta (syn_sm, 1), ~A2007~ (syn_a2007), W 40 / C 12
    (syn_c12), W 30 (tiny_a), W 20 / C 999 (1) and --no-rss (2: no pair mask, every structure all '.' with score L)."""
    m = io.read_model(gpath(model))
    seqs, quals = batch((3, 13, 40, 97, 131, 200), seed=len(model))
    eng = io.engine_from_model(m)
    eng.load_batch(seqs, quals)
    x = m["x"]
    _, xo = po.oracle_from_model(gpath(model))
    np.testing.assert_array_equal(x, xo)
    refs, res, mea = check_pair_path(eng, seqs, quals, x, lambda: po.oracle_from_model(gpath(model))[0], scan=True,
                                     no_rss=m["no_rss"])
    if m["no_rss"]:
        for g in GAMMAS:
            structs, scores, _ = mea[g]
            for seq, s, sc in zip(seqs, structs, scores):
                assert s == "." * len(seq) and sc == float(len(seq))
        assert all(len(r[2]) == 0 for r in res)
    else:
        assert sum(len(r[2]) for r in res) > 0


# ---- G. edge sequences

def edge_batch():
    """GGGAAAUCCC, all N (L 30), poly-A (L 40), L = 1 and 2 between live sequences of one group"""
    live_s, live_q = batch((60, 97, 131), seed=7)
    enc = {"A": 1, "C": 2, "G": 3, "U": 4}
    edge = [np.array([enc[c] for c in "GGGAAAUCCC"], dtype=np.uint8), np.zeros(30, dtype=np.uint8),
            np.ones(40, dtype=np.uint8), np.array([3], dtype=np.uint8), np.array([3, 2], dtype=np.uint8)]
    seqs = [live_s[0], edge[0], edge[1], live_s[1], edge[2], edge[3], live_s[2], edge[4]]
    quals = [live_q[0]] + [np.full(len(s) + 1, 10, dtype=np.uint8) for s in edge[:2]] + [live_q[1]] + \
            [np.full(len(s) + 1, 10, dtype=np.uint8) for s in edge[2:4]] + [live_q[2], np.full(3, 10, dtype=np.uint8)]
    for q in quals[1:3] + quals[4:6] + quals[7:]:
        q[-1] = 0
    return seqs, quals


@pytest.mark.parametrize("pattern", ["(.........)", P1])
def test_edge_sequences(pattern):
    """Sequences without a parse of the motif (Z(ari) = 0: the trainer skips them, but their parses without the motif keep
    their pairs) or without a kept pair, in one group with live sequences: `(.........)` cannot fit GGGAAAUCCC, whose G-C cells
    the filter keeps; all N and poly-A keep no cell (P: an empty list, unpaired exactly 1, an all-'.' structure of score L);
    L = 1, 2.  No NaN from 1 / Z or from a product of empty table entries, and their neighbours in the group stay exact."""
    seqs, quals = edge_batch()
    eng, x, refs, res, mea = run(pattern, seqs, quals, scan=True)
    kept0 = eng.pairs(1)[0]
    assert kept0.sum() > 0                                            # (GGGAAAUCCC keeps cells)
    for k in (2, 4):
        assert eng.pairs(k)[0].sum() == 0 and len(res[k][0]) == 0     # (all N / poly-A keep none)
        assert np.all(res[k][3] == 1.0) and mea[1.0][0][k] == "." * len(seqs[k]) and mea[1.0][1][k] == float(len(seqs[k]))
    if pattern == "(.........)":
        assert refs[1]["scan"]["exist_prob"] == 0.0 and len(res[1][0]) > 0
    assert all(refs[k]["P"] is not None for k in (0, 3, 6))


# ---- H. streamed batch

def test_streamed_batch_against_the_oracle():
    """max_resident 7: the batch runs in chunks of 7 sequences on inner engines, each with its own slots, P / M scratch and
    list, concatenated by stream_pairs with batch-global indices.  Lengths 40 .. 325 cross L = 256 inside a chunk and at chunk
    boundaries.  Against the oracle (the kept masks from a resident engine on the same batch: the filter does not depend on
    the streaming), not only against the resident batch."""
    lens = [40 + 15 * k for k in range(20)]
    seqs, quals = batch(lens, seed=77)
    resident = api.Engine(P1, PAR, 50, 30, 1e-4, 0.1, 0, 0)
    resident.load_batch(seqs, quals)
    x = perturbed(resident)
    eng = api.Engine(P1, PAR, 50, 30, 1e-4, 0.1, 0, 0)
    eng.set_option("max_resident", 7)
    eng.load_batch(seqs, quals)
    refs, res, _ = check_pair_path(eng, seqs, quals, x, oracle_maker(P1, 50, 30, x), scan=True, mask_eng=resident)
    assert sum(r["P"] is not None for r in refs) >= 18
