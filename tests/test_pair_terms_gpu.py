"""The pair terms of the outside train sweep (option pair_terms) on the GPU: the words the plan kernel builds
against the host entry (same rule functions, plan_rules.h); the train path with the option on against the oracle
(tests/train_check.py: fn, gr and the rows of every sequence); option 1 against 0 -- bit for bit in the deterministic mode, which
keeps its walk whatever the option says, within the tolerances of tests/test_useful_mask_gpu.py::compare in the default mode (the
dropped terms are exact zeros that were never added: only the order of the atomic adds differs); the kept zeros; the degenerate
batches; W = 64 and 65; and the scan records and debug_tables, which see no word.
Everything but the kept-zeros test runs under the NaN poisoning that tests/conftest.py turns on."""
import numpy as np
import pytest

from rnaelem_amd import api, synth
from tests import test_kept_zeros_gpu as kz
from tests import train_check as tc
from tests.test_pair_posterior_gpu import perturbed
from tests.test_pair_shapes_gpu import batch, oracle_maker
from tests.test_useful_mask_gpu import P1, P5, PAR, close_sums, compare, engine, has_dead_and_live_cells, ragged_batch

pytestmark = pytest.mark.gpu


def evaluate(eng, x, rows=True):
    res = eng.train_eval(x)
    return res, eng.seq_stats(), {k: v.copy() for k, v in eng.seq_counts().items()} if rows else None


def both_ways(eng, x, rows=True):
    """(train_eval, seq_stats, seq_counts) with the words on, then off"""
    out = []
    for on in (1, 0):
        eng.set_option("pair_terms", on)
        out.append(evaluate(eng, x, rows))
    eng.set_option("pair_terms", 1)
    return out


def popcount(words):
    return sum(bin(int(w)).count("1") for w in words[np.nonzero(words)])


@pytest.mark.parametrize("pattern", [P1, P5])
def test_gpu_words_equal_the_host_entry(pattern):
    seqs, quals = ragged_batch()
    eng = engine(pattern)
    eng.load_batch(seqs, quals)
    n_ha = n_h1 = 0
    for k in range(len(seqs)):
        mask, kept = eng.useful_mask(k), eng.pairs(k)[0]
        got, want = eng.pair_terms(k), api.pair_terms_host(mask, kept)
        for name, g, w in zip(("ha_rows", "h1_stems"), got, want):
            assert g.shape == w.shape == mask.shape
            assert np.array_equal(g, w), "sequence %d (L %d): %s differs in %d cells" % (k, len(seqs[k]), name, int((g != w).sum()))
        n_ha += popcount(got[0])
        n_h1 += popcount(got[1])
    print("%s: %d triples" % (pattern, n_ha))
    assert n_ha == n_h1 > 0 and not eng.pair_terms(17)[0].any() and not eng.pair_terms(17)[1].any()     # (17: the poly-A sequence)


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("pattern", [P1, P5])
def test_train_path_against_the_oracle_ragged(pattern, mode):
    seqs, quals = ragged_batch()
    eng = engine(pattern, opts=(("live_blocks", mode), ("pair_terms", 1)))
    eng.load_batch(seqs, quals)
    x = perturbed(eng)
    tc.check_train_path(eng, seqs, quals, x, oracle_maker(pattern, 50, 30, x))


@pytest.mark.parametrize("mode", [1, 2])
def test_train_path_against_the_oracle_l200(mode):
    seqs, quals = synth.synth_batch(3, 200)
    eng = engine(P1, opts=(("live_blocks", mode), ("pair_terms", 1)))
    eng.load_batch(seqs, quals)
    ha = eng.pair_terms(0)[0]
    ok = api.pair_terms_host(np.full_like(eng.useful_mask(0), 255), eng.pairs(0)[0])[0]
    print("L200 sequence 0: %d useful rows of %d parsable ones" % (popcount(ha), popcount(ok)))
    assert 0 < popcount(ha) < popcount(ok)
    x = perturbed(eng)
    tc.check_train_path(eng, seqs, quals, x, oracle_maker(P1, 50, 30, x))


CASES = {
    "ragged": (P1, 30, None, (), None),
    "ragged (.....)": (P5, 30, None, (), None),
    "ragged max_iloop 5": (P1, 5, None, (), None),
    "ragged lambda 0": (P1, 30, (0.0, 0.0), (), None),
    "ragged lambda 1": (P1, 30, (1.0, 1.0), (), None),
    "ragged window": (P1, 30, None, (), (5, 17)),
    "ragged streamed": (P1, 30, None, (("max_resident", 7),), None),
    "ragged live_blocks 2": (P1, 30, None, (("live_blocks", 2),), None),
    "ragged live_blocks 0": (P1, 30, None, (("live_blocks", 0),), None),
    "ragged loop_outside 0": (P1, 30, None, (("loop_outside", 0),), None),
}


@pytest.mark.parametrize("name", list(CASES))
def test_words_on_against_off(name):
    pattern, C, lam, opts, window = CASES[name]
    seqs, quals = ragged_batch()
    eng = engine(pattern, C, opts)
    eng.load_batch(seqs, quals)
    x = perturbed(eng)
    if lam is not None:
        x[-2:] = lam
    if window is not None:
        eng.set_option("eval_first", window[0])
        eng.set_option("eval_count", window[1])
    streamed = any(k == "max_resident" for k, _ in opts)
    for det in (1, 0):
        eng.set_option("deterministic", det)
        on, off = both_ways(eng, x, not streamed)
        compare(on, off, bool(det), "%s, deterministic %d" % (name, det))


def test_words_on_against_off_l200():
    seqs, quals = synth.synth_batch(3, 200)
    eng = engine()
    eng.load_batch(seqs, quals)
    x = perturbed(eng)
    for det in (1, 0):
        eng.set_option("deterministic", det)
        on, off = both_ways(eng, x)
        compare(on, off, bool(det), "3 x L200, deterministic %d" % det)


@pytest.mark.parametrize("lb", [1, 2])
def test_kept_zeros(lb):
    """no poisoning, a slot per sequence: the evaluations that keep the zeros of the dead entries, option 1 against option 0 (no
    field of the zeros' record names the option: the zeros one setting stored serve the other)"""
    eng = kz.engine(kz.CONFIGS[0], 1, (("live_blocks", lb),))
    eng.load_batch(*kz.BATCHES["A"])
    x0, x1 = kz.points(eng)
    first = evaluate(eng, x0)
    assert not eng.slot_status()["zeros_kept"]
    got = {}
    for on in (1, 0, 1):
        eng.set_option("pair_terms", on)
        for which, x in enumerate((x1, x0)):
            res = evaluate(eng, x)
            assert eng.slot_status()["zeros_kept"], (on, which)
            if (on, which) in got:
                compare(res, got[on, which], False, "pair_terms %d again, point %d" % (on, which))
            got[on, which] = res
    for which in (0, 1):
        compare(got[1, which], got[0, which], False, "kept zeros, live_blocks %d, point %d" % (lb, which))
    compare(got[1, 1], first, False, "keeping against storing")


def test_batch_without_a_live_cell():
    seqs, quals = ragged_batch()
    eng = engine()
    eng.load_batch(seqs[17:18], quals[17:18])
    assert not eng.useful_mask(0).any() and not eng.pair_terms(0)[0].any()
    on, off = both_ways(eng, perturbed(eng))
    compare(on, off, False, "no live cell")


def test_mask_of_all_ones_has_no_words():
    seqs, quals = ragged_batch()
    eng = engine(opts=(("useful_mask_lds_kb", 1),))
    eng.load_batch(seqs[:8], quals[:8])
    assert np.all(eng.useful_mask(0) == 255)
    with pytest.raises(api.ElemdpError):
        eng.pair_terms(0)
    for det in (1, 0):
        eng.set_option("deterministic", det)
        on, off = both_ways(eng, perturbed(eng))
        compare(on, off, bool(det), "mask of all ones, deterministic %d" % det)


def wide_engine(W):
    return api.Engine(P1, PAR, W, 30, 1e-4, 0.1, 0, 0)


def test_span_64_and_65():
    """a few sequences of L = 80.  W = 64: the words exist and use their upper bits (a bit >= 50 is set, asserted from the read-back);
    the train path against the oracle, and option 1 against 0.  W = 65: no words, option 1 is option 0."""
    seqs, quals = batch([80, 80, 80, 80], seed=7)
    eng = wide_engine(64)
    eng.load_batch(seqs, quals)
    top = 0
    for k in range(len(seqs)):
        mask, kept = eng.useful_mask(k), eng.pairs(k)[0]
        got, want = eng.pair_terms(k), api.pair_terms_host(mask, kept)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), k
        top = max(top, int(max(got[0].max(), got[1].max())).bit_length() - 1)
    print("W 64: highest bit %d" % top)
    assert top >= 50
    x = perturbed(eng)
    tc.check_train_path(eng, seqs, quals, x, oracle_maker(P1, 64, 30, x))
    for det in (1, 0):
        eng.set_option("deterministic", det)
        on, off = both_ways(eng, x)
        compare(on, off, bool(det), "W 64, deterministic %d" % det)
    eng = wide_engine(65)
    eng.load_batch(seqs, quals)
    with pytest.raises(api.ElemdpError):
        eng.pair_terms(0)
    x = perturbed(eng)
    for det in (1, 0):
        eng.set_option("deterministic", det)
        on, off = both_ways(eng, x)
        compare(on, off, bool(det), "W 65, deterministic %d" % det)


def test_scan_sees_no_word():
    seqs, quals = ragged_batch()
    eng = engine()
    eng.load_batch(seqs[:12], quals[:12])
    x = perturbed(eng)
    eng.train_eval(x)
    assert any(has_dead_and_live_cells(eng.useful_mask(k)) for k in range(12)) and any(eng.pair_terms(k)[0].any() for k in range(12))
    got = []
    for on in (1, 0):
        eng.set_option("pair_terms", on)
        got.append(eng.scan(x))
    (ra, ea), (rb, eb) = got
    np.testing.assert_allclose(ea, eb, rtol=1e-13, atol=1e-300, err_msg="scan: expected counts")
    for n, (a, b) in enumerate(zip(ra, rb)):
        assert (a["Ys"], a["Ye"], a["rss"]) == (b["Ys"], b["Ye"], b["rss"]) and np.array_equal(a["psihat"], b["psihat"]), n
        assert a["exist_prob"] == pytest.approx(b["exist_prob"], rel=1e-13), n
        for k in ("start", "inner", "end"):
            close_sums(a[k], b[k], "scan: sequence %d %s" % (n, k))


def test_debug_tables_see_no_word():
    seqs, quals = ragged_batch()
    eng = engine()
    eng.load_batch(seqs[3:4], quals[3:4])
    x = perturbed(eng)
    eng.train_eval(x)
    assert has_dead_and_live_cells(eng.useful_mask(0)) and eng.pair_terms(0)[0].any()
    eng.set_option("deterministic", 1)
    tabs = []
    for on in (1, 0):
        eng.set_option("pair_terms", on)
        eng.train_eval(x)
        tabs.append(eng.debug_tables())
    for k in tabs[0]:
        assert np.array_equal(tabs[0][k], tabs[1][k], equal_nan=True), k
