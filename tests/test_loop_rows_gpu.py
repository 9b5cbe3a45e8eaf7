"""k4_out_lrows (the seeds and the chain of the outside L plane in one kernel) at the shapes that
tests/test_loop_outside_gpu.py cannot reach -- every case there has W = 50, and W + 1 = 51 diagonals hide what a tile of T = 8
diagonals and a block of R rows do at their edges: band widths around the tile (a last tile of one, two, ... diagonals, a band
within one tile), sequence lengths around the block (a block of one row, a last block of one row, rows that end inside a tile),
against the sweep that computes L itself (loop_outside 0) at the tolerances of tests/test_useful_mask_gpu.py::compare, per
sequence against a batch of that sequence alone, and against the oracle; then schedule 0, a window and a streamed batch at such
a width.  Everything runs under the NaN poisoning that tests/conftest.py turns on: a seed the tile missed, or a parent row lost
between two tiles, shows as NaN in the statistics."""
import re

import numpy as np
import pytest

from rnaelem_amd import api
from tests import train_check as tc
from tests.test_loop_outside_gpu import both_ways
from tests.test_loop_prepass_gpu import hairpin_batch
from tests.test_pair_posterior_gpu import perturbed
from tests.test_pair_shapes_gpu import batch, oracle_maker
from tests.test_useful_mask_gpu import P1, P5, PAR, compare, ragged_batch

pytestmark = pytest.mark.gpu

T = 8                     # diagonals of a tile (kRowsT, lin_kernels.hip); the launcher's word is checked below
W_ODD = 2 * T + 3         # 20 diagonals: tiles of 8, 8 and 4


def engine(pattern, W, C=30, opts=()):
    eng = api.Engine(pattern, PAR, W, C, 1e-4, 0.1, 0, 0)
    for k, v in opts:
        eng.set_option(k, v)
    return eng


def block_shape(eng, x, capfd, monkeypatch):
    """(rows of a block, diagonals of a tile) of k4_out_lrows for the loaded batch, from the launcher's ELEMDP_LDS_DEBUG line"""
    monkeypatch.setenv("ELEMDP_LDS_DEBUG", "1")
    capfd.readouterr()
    eng.train_eval(x)
    got = re.findall(r"loop_outside 1 \(k4_out_lrows lds \d+, (\d+) rows x (\d+) diagonals\)", capfd.readouterr().err)
    monkeypatch.delenv("ELEMDP_LDS_DEBUG")
    assert got and len(set(got)) == 1, got
    return int(got[0][0]), int(got[0][1])


@pytest.mark.parametrize("C", [5, 30])
@pytest.mark.parametrize("W", [T - 2, T - 1, T, T + 3, 2 * T + 1, 3])
@pytest.mark.parametrize("pattern", [P1, P5])
def test_band_widths_around_the_tile(pattern, W, C):
    seqs, quals = ragged_batch()
    eng = engine(pattern, W, C)
    eng.load_batch(seqs, quals)
    x = perturbed(eng)
    on, off = both_ways(eng, x)
    compare(on, off, False, "%s W %d C %d" % (pattern, W, C))
    for pre in (0, 1):
        eng.set_option("loop_prepass", pre)
        on, off = both_ways(eng, x)
        compare(on, off, False, "%s W %d C %d loop_prepass %d" % (pattern, W, C, pre))


@pytest.mark.parametrize("pattern", [P1, P5])
def test_rows_around_the_block(pattern, capfd, monkeypatch):
    probe = engine(pattern, W_ODD)
    seqs, quals = batch([30], seed=3)
    probe.load_batch(seqs, quals)
    x = perturbed(probe)
    R, tile = block_shape(probe, x, capfd, monkeypatch)
    assert tile == T and 1 <= R <= 256
    # a block of one row (L = R: rows 0 .. R), a last block of one row, rows on either side of it, three blocks; and sequences
    # shorter than the band, whose rows all end before the top diagonal
    lens = [1, R - 1, R, R + 1, 2 * R + 1, 2, 5, T, W_ODD - 1, W_ODD, W_ODD + 1, 3 * R + 7]
    seqs, quals = batch(lens, seed=23)
    eng = engine(pattern, W_ODD)
    eng.load_batch(seqs, quals)
    on, off = both_ways(eng, x)
    compare(on, off, False, "%s rows around a block of %d" % (pattern, R))
    one = engine(pattern, W_ODD)
    for k in range(len(seqs)):
        one.load_batch(seqs[k:k + 1], quals[k:k + 1])
        one.train_eval(x)
        np.testing.assert_allclose(on[1][k], one.seq_stats()[0], rtol=1e-10, atol=1e-10, err_msg="sequence %d (L %d) alone" % (k, lens[k]))


@pytest.mark.parametrize("pattern", [P1, P5])
def test_train_path_against_the_oracle_at_a_band_of_three_tiles(pattern):
    seqs, quals = hairpin_batch()
    eng = engine(pattern, W_ODD, opts=(("loop_outside", 1),))
    eng.load_batch(seqs, quals)
    x = perturbed(eng)
    tc.check_train_path(eng, seqs, quals, x, oracle_maker(pattern, W_ODD, 30, x))


def test_schedule_0():
    seqs, quals = ragged_batch()
    eng = engine(P1, W_ODD, opts=(("schedule", 0),))
    eng.load_batch(seqs, quals)
    x = perturbed(eng)
    on, off = both_ways(eng, x)
    compare(on, off, False, "schedule 0")


def test_window_and_streamed_batch():
    seqs, quals = ragged_batch()
    eng = engine(P1, W_ODD)
    eng.load_batch(seqs, quals)
    x = perturbed(eng)
    eng.train_eval(x)
    whole = eng.seq_stats().copy()
    eng.set_option("eval_first", 5)
    eng.set_option("eval_count", 17)
    on, off = both_ways(eng, x)
    compare(on, off, False, "window")
    np.testing.assert_allclose(on[1][5:22], whole[5:22], rtol=1e-10, atol=1e-10, err_msg="window against the whole batch")
    st = engine(P1, W_ODD, opts=(("max_resident", 7),))
    st.load_batch(seqs, quals)
    on, off = both_ways(st, x, rows=False)
    compare(on, off, False, "streamed")
    np.testing.assert_allclose(on[1], whole, rtol=1e-10, atol=1e-10, err_msg="streamed against the resident batch")
