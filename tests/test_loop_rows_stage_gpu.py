"""k4_out_lrows stages its plan data once per workgroup (the mask bytes of its rows, their pair-mask words,
base and weight of its positions, the runs of records of every tile), and a record names its own cell.  tests/test_loop_rows_gpu.py
walks the edges of tiles and blocks; the cases here are what staging once can get wrong: sequences of very different lengths in
one launch (a short one's blocks return early, its window of positions clips at L), rows that end before the top diagonal
(L <= W: run bounds beyond the row), both patterns (their L rows differ in width, so the blocks differ in rows), the widest and
the narrowest run of pair-mask words (W = 64 and 3), C = 5 and 30, sequences without a kept pair (empty runs, all bounds
equal), N bases, schedule 0, a ranged evaluation, a streamed batch -- and a band so wide that the staged data no longer fit the
workgroup's LDS, where the sweep must compute L itself.  Every case compares loop_outside 1 against 0 at the tolerances of
tests/test_useful_mask_gpu.py::compare, under the NaN poisoning that tests/conftest.py turns on."""
import re

import numpy as np
import pytest

from tests.test_loop_outside_gpu import both_ways
from tests.test_loop_rows_gpu import block_shape, engine
from tests.test_pair_posterior_gpu import perturbed
from tests.test_pair_shapes_gpu import batch
from tests.test_useful_mask_gpu import P1, P5, compare, ragged_batch

pytestmark = pytest.mark.gpu

LDS_MAX = 64 * 1024       # kLoopRowsLdsMax (loop_rows_layout.h): beyond it the sweep computes L itself


def path_taken(eng, x, capfd, monkeypatch):
    """(loop_outside as the launcher decided it, the LDS bytes k4_out_lrows would take) from the ELEMDP_LDS_DEBUG line of one
    evaluation with the option on"""
    monkeypatch.setenv("ELEMDP_LDS_DEBUG", "1")
    eng.set_option("loop_outside", 1)
    capfd.readouterr()
    eng.train_eval(x)
    got = re.findall(r"loop_outside (\d) \(k4_out_lrows lds (\d+), \d+ rows x \d+ diagonals\)", capfd.readouterr().err)
    monkeypatch.delenv("ELEMDP_LDS_DEBUG")
    assert got and len(set(got)) == 1, got
    return int(got[0][0]), int(got[0][1])


@pytest.mark.parametrize("pattern", [P1, P5])
def test_different_lengths_in_one_launch(pattern, capfd, monkeypatch):
    probe = engine(pattern, 50)
    seqs, quals = batch([30], seed=3)
    probe.load_batch(seqs, quals)
    x = perturbed(probe)
    R, _ = block_shape(probe, x, capfd, monkeypatch)
    lens = [1, R - 1, R + 1, 2 * R + 1, 3 * R + 7]
    seqs, quals = batch(lens, seed=29)
    eng = engine(pattern, 50)
    eng.load_batch(seqs, quals)
    assert path_taken(eng, x, capfd, monkeypatch)[0] == 1
    on, off = both_ways(eng, x)
    compare(on, off, False, "%s lengths %s in one launch" % (pattern, lens))
    one = engine(pattern, 50)
    for k in range(len(seqs)):
        one.load_batch(seqs[k:k + 1], quals[k:k + 1])
        one.train_eval(x)
        np.testing.assert_allclose(on[1][k], one.seq_stats()[0], rtol=1e-10, atol=1e-10, err_msg="sequence %d (L %d) alone" % (k, lens[k]))


@pytest.mark.parametrize("C", [5, 30])
@pytest.mark.parametrize("W", [64, 3])
@pytest.mark.parametrize("pattern", [P1, P5])
def test_widest_and_narrowest_band(pattern, W, C, capfd, monkeypatch):
    # (the ragged batch: L from 20 to 120, so rows that end before the top diagonal of W = 64 and rows that reach it; N bases in
    # every third sequence, one poly-A, both labels)
    seqs, quals = ragged_batch()
    eng = engine(pattern, W, C)
    eng.load_batch(seqs, quals)
    x = perturbed(eng)
    assert path_taken(eng, x, capfd, monkeypatch)[0] == 1
    on, off = both_ways(eng, x)
    compare(on, off, False, "%s W %d C %d" % (pattern, W, C))


@pytest.mark.parametrize("pattern", [P1, P5])
def test_sequences_shorter_than_the_band(pattern):
    seqs, quals = batch([2, 9, 17, 33, 49, 50, 51], seed=31)
    eng = engine(pattern, 50)
    eng.load_batch(seqs, quals)
    x = perturbed(eng)
    on, off = both_ways(eng, x)
    compare(on, off, False, "%s L <= W" % pattern)


def test_no_kept_pair_and_n_bases():
    # poly-A sequences keep no pair: every run of records is empty and all its bounds are equal
    lens = [7, 40, 64, 90]
    seqs = [np.full(L, 1, dtype=np.uint8) for L in lens]
    quals = [np.append(np.full(L, 10, dtype=np.uint8), np.uint8(5 * (k % 2))) for k, L in enumerate(lens)]
    eng = engine(P1, 50)
    eng.load_batch(seqs, quals)
    x = perturbed(eng)
    on, off = both_ways(eng, x)
    compare(on, off, False, "poly-A")
    # N bases in every sequence
    seqs, quals = batch([25, 60, 61, 110], seed=37, n_every=1)
    assert all((s == 0).any() for s in seqs)
    eng.load_batch(seqs, quals)
    on, off = both_ways(eng, x)
    compare(on, off, False, "N bases")


def test_schedule_0_window_and_streamed_batch():
    seqs, quals = ragged_batch()
    eng = engine(P1, 64, opts=(("schedule", 0),))
    eng.load_batch(seqs, quals)
    x = perturbed(eng)
    on, off = both_ways(eng, x)
    compare(on, off, False, "schedule 0")
    eng = engine(P1, 64)
    eng.load_batch(seqs, quals)
    eng.train_eval(x)
    whole = eng.seq_stats().copy()
    eng.set_option("eval_first", 11)
    eng.set_option("eval_count", 9)
    on, off = both_ways(eng, x)
    compare(on, off, False, "a ranged evaluation")
    np.testing.assert_allclose(on[1][11:20], whole[11:20], rtol=1e-10, atol=1e-10, err_msg="the range against the whole batch")
    st = engine(P1, 64, opts=(("max_resident", 9),))
    st.load_batch(seqs, quals)
    on, off = both_ways(st, x, rows=False)
    compare(on, off, False, "streamed")
    np.testing.assert_allclose(on[1], whole, rtol=1e-10, atol=1e-10, err_msg="streamed against the resident batch")


@pytest.mark.parametrize("W,L,kernel", [(120, 130, 1), (600, 610, 0)])
def test_a_width_that_must_fall_back(W, L, kernel, capfd, monkeypatch):
    """the layout decides per band width: at W = 120 the staged plan data still fit and the kernel runs, at W = 600 they outgrow
    the 64 KiB of a workgroup and the sweep computes L itself; either way the results are those of loop_outside 0"""
    seqs, quals = batch([L, 40], seed=41, n_every=0)
    eng = engine(P1, W)
    eng.load_batch(seqs, quals)
    x = perturbed(eng)
    ran, lds = path_taken(eng, x, capfd, monkeypatch)
    assert (lds <= LDS_MAX) == bool(kernel), (W, lds)
    assert ran == kernel, (W, ran, lds)
    on, off = both_ways(eng, x)
    compare(on, off, False, "W %d L %d (k4_out_lrows ran: %d)" % (W, L, ran))
