"""The live-block lists of the train sweeps on the GPU: the lists the plan kernel builds against the host
entry (same rule function, live_blocks.h); the train path with the lists against the oracle (tests/train_check.py: fn, gr and the
rows of every sequence); option live_blocks 1 against 0 within the tolerances of tests/test_useful_mask_gpu.py::compare in the
default mode, and bit for bit in the deterministic mode, which keeps consecutive cells whatever the option says; the degenerate
masks (no live cell at all; all ones); and the scan records and debug_tables, which see no list.
Option value 1 (the default) takes the lists on the diagonals where the plan finds that they leave fewer workgroups and keeps
consecutive cells on the others -- both kernel forms in one sweep, the consecutive one with the window of the list form; the tests
assert from the read-back that the batch has diagonals of either kind.  Value 2 takes lists on every diagonal: the train path is
held to the same checks under both, so that every diagonal of these small batches is swept from lists once.
Everything runs under the NaN poisoning that tests/conftest.py turns on: an entry that the listed sweeps left unstored and that
somebody reads would show as NaN."""
import numpy as np
import pytest

from rnaelem_amd import api, synth
from tests import train_check as tc
from tests.test_pair_posterior_gpu import perturbed
from tests.test_pair_shapes_gpu import oracle_maker
from tests.test_useful_mask_gpu import P1, P5, close_sums, compare, engine, has_dead_and_live_cells, ragged_batch

pytestmark = pytest.mark.gpu


def diagonals_with_lists(eng, mode, k=None):
    """which diagonals the train sweeps of the engine's options take from lists (read-back of the plan; sequence k, default the
    longest of the resident batch); asserts what the option value promises: 2 every diagonal, 0 none"""
    if k is None:
        k = int(np.argmax(np.diff(eng._off)))
    taken = eng.live_blocks(k, with_taken=True)[3]
    if mode == 2:
        assert taken.all()
    if mode == 0:
        assert not taken.any()
    return taken


@pytest.mark.parametrize("span", [0, 16])
@pytest.mark.parametrize("pattern", [P1, P5])
def test_gpu_lists_equal_the_host_entry(pattern, span):
    seqs, quals = ragged_batch()
    eng = engine(pattern, opts=(("live_span", span),))
    eng.load_batch(seqs, quals)
    n_blocks = n_gaps = 0
    for k in range(len(seqs)):
        got, cpb, cap = eng.live_blocks(k)
        assert cpb >= 8 and cap == max(cpb, span if span else 32), (cpb, cap)      # (never below the cells of a block)
        want = api.live_blocks_host(eng.useful_mask(k), cpb, cap)
        assert got == want, "sequence %d (L %d)" % (k, len(seqs[k]))
        n_blocks += sum(len(row) for row in got)
        n_gaps += sum(cells[-1] - first + 1 > len(cells) for row in got for first, cells, _ in row)
    print("%s span %d: %d blocks, %d with gaps" % (pattern, span, n_blocks, n_gaps))
    assert n_blocks > 0 and n_gaps > 0
    assert all(row == [] for row in eng.live_blocks(17)[0])        # (the poly-A sequence: no live cell, no block)


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("pattern", [P1, P5])
def test_train_path_against_the_oracle_ragged(pattern, mode):
    seqs, quals = ragged_batch()
    eng = engine(pattern, opts=(("live_blocks", mode),))
    eng.load_batch(seqs, quals)
    x = perturbed(eng)
    tc.check_train_path(eng, seqs, quals, x, oracle_maker(pattern, 50, 30, x))
    taken = diagonals_with_lists(eng, mode)
    print("%s live_blocks %d: lists on the diagonals %s" % (pattern, mode, np.flatnonzero(taken).tolist()))
    if mode == 1:       # the default sweeps this batch with both kernel forms
        assert taken.any() and not taken.all()


@pytest.mark.parametrize("mode", [1, 2])
def test_train_path_against_the_oracle_where_the_span_closes_blocks(mode):
    """three sequences of L = 200: the smallest shape at which the default span closes blocks (asserted)"""
    seqs, quals = synth.synth_batch(3, 200)
    eng = engine(P1, opts=(("live_blocks", mode),))
    eng.load_batch(seqs, quals)
    closed = 0
    for k in range(3):
        lists, cpb, _ = eng.live_blocks(k)
        closed += sum(len(cells) < cpb and b + 1 < len(row) for row in lists for b, (_, cells, _) in enumerate(row))
    assert closed > 0
    x = perturbed(eng)
    tc.check_train_path(eng, seqs, quals, x, oracle_maker(P1, 50, 30, x))
    taken = diagonals_with_lists(eng, mode)
    print("3 x L200 live_blocks %d: lists on the diagonals %s" % (mode, np.flatnonzero(taken).tolist()))
    if mode == 1:
        assert taken.any() and not taken.all()


def both_ways(eng, x, rows=True, mode=1):
    """(train_eval, seq_stats, seq_counts) with the lists on, then off"""
    out = []
    for on in (mode, 0):
        eng.set_option("live_blocks", on)
        res = eng.train_eval(x)
        out.append((res, eng.seq_stats(), {k: v.copy() for k, v in eng.seq_counts().items()} if rows else None))
    eng.set_option("live_blocks", 1)
    return out


CASES = {
    "ragged": (P1, 30, None, (), None),
    "ragged (.....)": (P5, 30, None, (), None),
    "ragged max_iloop 5": (P1, 5, None, (), None),
    "ragged lambda 0": (P1, 30, (0.0, 0.0), (), None),
    "ragged lambda 1": (P1, 30, (1.0, 1.0), (), None),
    "ragged window": (P1, 30, None, (), (5, 17)),
    "ragged streamed": (P1, 30, None, (("max_resident", 7),), None),
    "ragged live_span 16": (P1, 30, None, (("live_span", 16),), None),
}


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("name", list(CASES))
def test_lists_on_against_off(name, mode):
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
        on, off = both_ways(eng, x, not streamed, mode)
        compare(on, off, bool(det), "%s, live_blocks %d, deterministic %d" % (name, mode, det))
    if not streamed:      # (default mode, the option back at 1: which diagonals took lists)
        eng.set_option("live_blocks", mode)
        taken = diagonals_with_lists(eng, mode)
        if mode == 1:
            assert taken.any() and not taken.all(), name
        eng.set_option("deterministic", 1)
        assert not diagonals_with_lists(eng, 0).any()       # (the deterministic mode keeps consecutive cells)


def test_batch_without_a_live_cell():
    """only the poly-A sequence: no block on any diagonal; the evaluation is finite and equals the one without lists"""
    seqs, quals = ragged_batch()
    eng = engine()
    eng.load_batch(seqs[17:18], quals[17:18])
    assert not eng.useful_mask(0).any() and all(row == [] for row in eng.live_blocks(0)[0])
    for mode in (1, 2):
        on, off = both_ways(eng, perturbed(eng), mode=mode)
        compare(on, off, False, "no live cell, live_blocks %d" % mode)


def test_mask_of_all_ones_gives_consecutive_blocks():
    seqs, quals = ragged_batch()
    eng = engine(opts=(("useful_mask_lds_kb", 1),))
    eng.load_batch(seqs[:8], quals[:8])
    for k in range(8):
        assert np.all(eng.useful_mask(k) == 255), k
        lists, cpb, _ = eng.live_blocks(k)
        L = len(seqs[k])
        for d, row in enumerate(lists):
            ncell = L - d + 1
            assert [cells for _, cells, _ in row] == [list(range(i, min(i + cpb, ncell))) for i in range(0, ncell, cpb)], (k, d)
    for mode in (1, 2):
        on, off = both_ways(eng, perturbed(eng), mode=mode)
        compare(on, off, False, "mask of all ones, live_blocks %d" % mode)


def test_scan_sees_no_list():
    """a train evaluation in the default mode first, which builds the plan's lists and sweeps some diagonals from them; then the
    scan with the option 1 and 0"""
    seqs, quals = ragged_batch()
    eng = engine()
    eng.load_batch(seqs[:12], quals[:12])
    x = perturbed(eng)
    eng.train_eval(x)
    assert any(has_dead_and_live_cells(eng.useful_mask(k)) for k in range(12))
    assert diagonals_with_lists(eng, 1).any() and any(row for row in eng.live_blocks(0)[0])
    got = []
    for on in (1, 0):
        eng.set_option("live_blocks", on)
        got.append(eng.scan(x))
    (ra, ea), (rb, eb) = got
    np.testing.assert_allclose(ea, eb, rtol=1e-13, atol=1e-300, err_msg="scan: expected counts")
    for n, (a, b) in enumerate(zip(ra, rb)):
        assert (a["Ys"], a["Ye"], a["rss"]) == (b["Ys"], b["Ye"], b["rss"]) and np.array_equal(a["psihat"], b["psihat"]), n
        assert a["exist_prob"] == pytest.approx(b["exist_prob"], rel=1e-13), n
        for k in ("start", "inner", "end"):
            close_sums(a[k], b[k], "scan: sequence %d %s" % (n, k))


def test_debug_tables_see_no_list():
    """debug_tables repeats the evaluation of one sequence with the generic kernels, which take no list: once the plan holds lists
    (a train evaluation in the default mode), its tables in the deterministic mode are identical with the option 1 and 0"""
    seqs, quals = ragged_batch()
    eng = engine()
    eng.load_batch(seqs[3:4], quals[3:4])
    x = perturbed(eng)
    eng.train_eval(x)
    assert has_dead_and_live_cells(eng.useful_mask(0)) and diagonals_with_lists(eng, 1).any()
    eng.set_option("deterministic", 1)
    tabs = []
    for on in (1, 0):
        eng.set_option("live_blocks", on)
        eng.train_eval(x)
        tabs.append(eng.debug_tables())
    for k in tabs[0]:
        assert np.array_equal(tabs[0][k], tabs[1][k], equal_nan=True), k
