"""The row pre-pass of the inside L plane (option loop_prepass) on the GPU: the table-driven train sweep
behind the pre-pass against the sweep that computes L itself -- bit for bit in the deterministic mode (every stored L entry is the
same double, and L enters no heavy sum), within the tolerances of tests/test_useful_mask_gpu.py::compare in the default mode --
for live_blocks 0, 1 and 2 and live_span 12 and 32; against the oracle on a ragged batch around the first hairpin (L = 1 .. 7),
below and above the band width, with a sequence without a kept pair, one with N bases and one of L = 200; a window, a streamed
batch and the mask of all ones; the scan, debug_tables and a sample, which see neither list nor pre-pass; and the read-back of the
inside lists against the host rule.
Everything runs under the NaN poisoning that tests/conftest.py turns on: an L entry the pre-pass missed shows as NaN in whatever
reads it."""
import numpy as np
import pytest

from rnaelem_amd import api
from tests import train_check as tc
from tests.test_pair_posterior_gpu import perturbed
from tests.test_pair_shapes_gpu import batch, oracle_maker
from tests.test_useful_mask_gpu import P1, P5, close_sums, compare, engine, ragged_batch

pytestmark = pytest.mark.gpu


def both_ways(eng, x, rows=True):
    """(train_eval, seq_stats, seq_counts) with the pre-pass, then without"""
    out = []
    for on in (1, 0):
        eng.set_option("loop_prepass", on)
        res = eng.train_eval(x)
        out.append((res, eng.seq_stats(), {k: v.copy() for k, v in eng.seq_counts().items()} if rows else None))
    eng.set_option("loop_prepass", 1)
    return out


@pytest.mark.parametrize("span", [12, 32])
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("pattern", [P1, P5])
def test_prepass_on_against_off(pattern, mode, span):
    seqs, quals = ragged_batch()
    eng = engine(pattern, opts=(("live_blocks", mode), ("live_span", span)))
    eng.load_batch(seqs, quals)
    x = perturbed(eng)
    for det in (1, 0):
        eng.set_option("deterministic", det)
        on, off = both_ways(eng, x)
        compare(on, off, bool(det), "%s live_blocks %d live_span %d deterministic %d" % (pattern, mode, span, det))
    # which diagonals the inside sweep took from its own lists: none below the first hairpin, none without the pre-pass
    k = int(np.argmax(np.diff(eng._off)))
    taken = eng.live_blocks(k, with_taken=True, inside=True)[3]
    assert not taken[:3].any()
    if mode != 1:          # (1: the plan's choice per diagonal, which a span of the cells per block may leave without any list)
        assert taken[3:].all() if mode == 2 else not taken.any()
    eng.set_option("loop_prepass", 0)
    assert not eng.live_blocks(k, with_taken=True, inside=True)[3].any()
    eng.set_option("loop_prepass", 1)
    eng.set_option("deterministic", 1)
    assert not eng.live_blocks(k, with_taken=True, inside=True)[3].any()


def hairpin_batch():
    """L = 1, 2, 4, 5, 6, 7 (the first E cell, d = 3, reads a pre-passed L row under a pair of span 5), lengths below, at and above
    the band width 50, a poly-A sequence (no kept pair), sequences with N bases (every third of `batch`), and one of L = 200"""
    lens = [1, 2, 4, 5, 6, 7, 9, 23, 49, 50, 51, 64, 65, 97, 200]
    seqs, quals = batch(lens, seed=11)
    enc = {"A": 1, "C": 2, "G": 3, "U": 4}
    for k, s in ((3, "GAAAC"), (4, "GGAAAC"), (5, "GCAAAGC")):        # (pairs of the smallest spans, so that the short ones parse)
        seqs[k] = np.array([enc[c] for c in s], dtype=np.uint8)
    seqs.insert(8, np.full(50, 1, dtype=np.uint8))
    quals.insert(8, np.append(np.full(50, 10, dtype=np.uint8), np.uint8(0)))
    return seqs, quals


@pytest.mark.parametrize("pattern", [P1, P5])
def test_train_path_against_the_oracle_around_the_first_hairpin(pattern):
    seqs, quals = hairpin_batch()
    eng = engine(pattern)
    eng.load_batch(seqs, quals)
    assert any((s == 0).any() for s in seqs) and eng.pairs(8)[0].sum() == 0 and not eng.useful_mask(8).any()
    assert max(len(s) for s in seqs) == 200 and min(len(s) for s in seqs) == 1
    x = perturbed(eng)
    tc.check_train_path(eng, seqs, quals, x, oracle_maker(pattern, 50, 30, x))


def test_window_and_streamed_batch_give_the_rows_of_the_whole_batch():
    seqs, quals = ragged_batch()
    eng = engine()
    eng.load_batch(seqs, quals)
    x = perturbed(eng)
    eng.set_option("deterministic", 1)
    eng.train_eval(x)
    whole = eng.seq_stats().copy()
    eng.set_option("eval_first", 5)
    eng.set_option("eval_count", 17)
    on, off = both_ways(eng, x)
    compare(on, off, True, "window")
    np.testing.assert_allclose(on[1][5:22], whole[5:22], rtol=1e-10, atol=1e-10, err_msg="window against the whole batch")
    st = engine(opts=(("max_resident", 7), ("deterministic", 1)))
    st.load_batch(seqs, quals)
    on, off = both_ways(st, x, rows=False)
    compare(on, off, True, "streamed")
    np.testing.assert_allclose(on[1], whole, rtol=1e-10, atol=1e-10, err_msg="streamed against the resident batch")


def test_mask_of_all_ones_gives_consecutive_inside_blocks():
    seqs, quals = ragged_batch()
    eng = engine(opts=(("useful_mask_lds_kb", 1),))
    eng.load_batch(seqs[:8], quals[:8])
    for k in range(8):
        assert np.all(eng.useful_mask(k) == 255), k
        lists, cpb, _ = eng.live_blocks(k, inside=True)
        L = len(seqs[k])
        for d, row in enumerate(lists):
            ncell = L - d + 1
            assert [cells for _, cells, _ in row] == [list(range(i, min(i + cpb, ncell))) for i in range(0, ncell, cpb)], (k, d)
    x = perturbed(eng)
    for det in (1, 0):
        eng.set_option("deterministic", det)
        on, off = both_ways(eng, x)
        compare(on, off, bool(det), "mask of all ones, deterministic %d" % det)


def test_inside_read_back_equals_the_host_rule():
    seqs, quals = ragged_batch()
    n_less = 0
    for span in (0, 12):
        eng = engine(opts=(("live_span", span),))
        eng.load_batch(seqs, quals)
        for k in range(len(seqs)):
            got, cpb, cap, taken = eng.live_blocks(k, with_taken=True, inside=True)
            mask = eng.useful_mask(k)
            assert got == api.live_blocks_host(mask, cpb, cap, bits=api.LIVE_INSIDE_BITS), (span, k)
            assert all(row == [] for row in got[:3]) and not taken[:3].any(), (span, k)
            whole = eng.live_blocks(k)[0]
            assert whole == api.live_blocks_host(mask, cpb, cap), (span, k)          # (the first set is what it was)
            n_less += sum(len(r) for r in got) < sum(len(r) for r in whole)
    assert n_less > 0


def test_scan_debug_tables_and_sample_see_no_prepass():
    """after a train evaluation behind the pre-pass (which builds both sets of lists): the scan and a sample with the option 1 and
    0, and debug_tables of one sequence in the deterministic mode"""
    seqs, quals = ragged_batch()
    eng = engine()
    eng.load_batch(seqs[:12], quals[:12])
    x = perturbed(eng)
    eng.train_eval(x)
    got, smp = [], []
    for on in (1, 0):
        eng.set_option("loop_prepass", on)
        got.append(eng.scan(x))
        smp.append(eng.sample_structures(x, 3, seed=5))
    (ra, ea), (rb, eb) = got
    np.testing.assert_allclose(ea, eb, rtol=1e-13, atol=1e-300, err_msg="scan: expected counts")
    for n, (a, b) in enumerate(zip(ra, rb)):
        assert (a["Ys"], a["Ye"], a["rss"]) == (b["Ys"], b["Ye"], b["rss"]) and np.array_equal(a["psihat"], b["psihat"]), n
        for k in ("start", "inner", "end"):
            close_sums(a[k], b[k], "scan: sequence %d %s" % (n, k))
    for n, (a, b) in enumerate(zip(*smp)):          # (rss, nodes, logp, status) per sequence
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[3], b[3]), n
        np.testing.assert_allclose(a[2], b[2], rtol=1e-12, atol=0, err_msg="logp of sequence %d" % n)      # (sums of atomics)
    one = engine()
    one.load_batch(seqs[3:4], quals[3:4])
    one.set_option("deterministic", 1)
    tabs = []
    for on in (1, 0):
        one.set_option("loop_prepass", on)
        one.train_eval(x)
        tabs.append(one.debug_tables())
    for k in tabs[0]:
        assert np.array_equal(tabs[0][k], tabs[1][k], equal_nan=True), k
