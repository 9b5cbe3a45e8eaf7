"""The outside L plane behind the sweep (option loop_outside) on the GPU: the table-driven train sweep in
front of k4_out_seed / k4_out_loops against the sweep that computes L itself, within the default-mode tolerances of
tests/test_useful_mask_gpu.py::compare (the heavy sums and the statistics are sums of atomics in either form) -- for live_blocks
0, 1 and 2, live_span 12 and 32, with and without the inside pre-pass -- and bit for bit in the deterministic mode, where the
option is ignored; against the oracle on the ragged batch around the first hairpin; a window, a streamed batch, the mask of all
ones and schedule 0 (two outside passes, the L kernels behind each); the launcher's own word that the L kernels ran; and the
scan, a sample and debug_tables, which see nothing of it.
Everything runs under the NaN poisoning that tests/conftest.py turns on: an L entry the seed kernel missed, or an E entry the
sweep left to a skipped cell, shows as NaN in the statistics of the chain kernel."""
import numpy as np
import pytest

from tests import train_check as tc
from tests.test_loop_prepass_gpu import hairpin_batch
from tests.test_pair_posterior_gpu import perturbed
from tests.test_pair_shapes_gpu import oracle_maker
from tests.test_useful_mask_gpu import P1, P5, close_sums, compare, engine, ragged_batch

pytestmark = pytest.mark.gpu


def both_ways(eng, x, rows=True):
    """(train_eval, seq_stats, seq_counts) with the L plane behind the sweep, then with the sweep that computes it"""
    out = []
    for on in (1, 0):
        eng.set_option("loop_outside", on)
        res = eng.train_eval(x)
        out.append((res, eng.seq_stats(), {k: v.copy() for k, v in eng.seq_counts().items()} if rows else None))
    eng.set_option("loop_outside", 1)
    return out


@pytest.mark.parametrize("span", [12, 32])
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("pattern", [P1, P5])
def test_outside_on_against_off(pattern, mode, span):
    seqs, quals = ragged_batch()
    eng = engine(pattern, opts=(("live_blocks", mode), ("live_span", span)))
    eng.load_batch(seqs, quals)
    x = perturbed(eng)
    for pre in (1, 0):          # (without the pre-pass the second set of lists is built for the outside sweep alone)
        eng.set_option("loop_prepass", pre)
        for det in (1, 0):
            eng.set_option("deterministic", det)
            on, off = both_ways(eng, x)
            compare(on, off, bool(det), "%s live_blocks %d live_span %d loop_prepass %d deterministic %d" % (pattern, mode, span, pre, det))


@pytest.mark.parametrize("pre", [1, 0])
@pytest.mark.parametrize("pattern", [P1, P5])
def test_the_l_kernels_run_where_the_option_is_on(pattern, pre, capfd, monkeypatch):
    """what the launcher decided, from its ELEMDP_LDS_DEBUG line (the flag behind its own gates: lists of the inside set built, the
    automaton fit for the L kernels): on in the default mode with and without the inside pre-pass, off with the option 0 and in
    the deterministic mode -- so that the comparisons of this file cannot pass by running the parent's path twice"""
    import re
    monkeypatch.setenv("ELEMDP_LDS_DEBUG", "1")
    seqs, quals = ragged_batch()
    eng = engine(pattern, opts=(("loop_prepass", pre),))
    eng.load_batch(seqs, quals)
    x = perturbed(eng)

    def flags():
        capfd.readouterr()
        eng.train_eval(x)
        got = re.findall(r"loop_prepass (\d) loop_outside (\d)", capfd.readouterr().err)
        assert got and len(set(got)) == 1, got
        return tuple(int(v) for v in got[0])

    assert flags() == (pre, 1)
    eng.set_option("loop_outside", 0)
    assert flags() == (pre, 0)
    eng.set_option("loop_outside", 1)
    eng.set_option("deterministic", 1)
    assert flags() == (pre, 0)
    eng.set_option("deterministic", 0)
    assert flags() == (pre, 1)


@pytest.mark.parametrize("pattern", [P1, P5])
def test_train_path_against_the_oracle_around_the_first_hairpin(pattern):
    seqs, quals = hairpin_batch()
    eng = engine(pattern, opts=(("loop_outside", 1),))
    eng.load_batch(seqs, quals)
    assert max(len(s) for s in seqs) == 200 and min(len(s) for s in seqs) == 1
    x = perturbed(eng)
    tc.check_train_path(eng, seqs, quals, x, oracle_maker(pattern, 50, 30, x))


def test_window_and_streamed_batch_give_the_rows_of_the_whole_batch():
    seqs, quals = ragged_batch()
    eng = engine()
    eng.load_batch(seqs, quals)
    x = perturbed(eng)
    eng.train_eval(x)
    whole = eng.seq_stats().copy()
    eng.set_option("eval_first", 5)
    eng.set_option("eval_count", 17)
    on, off = both_ways(eng, x)
    compare(on, off, False, "window")
    np.testing.assert_allclose(on[1][5:22], whole[5:22], rtol=1e-10, atol=1e-10, err_msg="window against the whole batch")
    st = engine(opts=(("max_resident", 7),))
    st.load_batch(seqs, quals)
    on, off = both_ways(st, x, rows=False)
    compare(on, off, False, "streamed")
    np.testing.assert_allclose(on[1], whole, rtol=1e-10, atol=1e-10, err_msg="streamed against the resident batch")


def test_mask_of_all_ones():
    seqs, quals = ragged_batch()
    eng = engine(opts=(("useful_mask_lds_kb", 1),))
    eng.load_batch(seqs[:8], quals[:8])
    assert all(np.all(eng.useful_mask(k) == 255) for k in range(8))
    x = perturbed(eng)
    on, off = both_ways(eng, x)
    compare(on, off, False, "mask of all ones")


def test_schedule_0_runs_the_l_kernels_behind_each_pass():
    seqs, quals = ragged_batch()
    eng = engine(opts=(("schedule", 0),))
    eng.load_batch(seqs, quals)
    x = perturbed(eng)
    on, off = both_ways(eng, x)
    compare(on, off, False, "schedule 0")


def test_scan_debug_tables_and_sample_see_no_change():
    seqs, quals = ragged_batch()
    eng = engine()
    eng.load_batch(seqs[:12], quals[:12])
    x = perturbed(eng)
    eng.train_eval(x)
    got, smp = [], []
    for on in (1, 0):
        eng.set_option("loop_outside", on)
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
    tabs = []
    for on in (1, 0):
        one.set_option("loop_outside", on)
        one.train_eval(x)
        tabs.append(one.debug_tables())
    for k in tabs[0]:          # (the generic kernels repeat the evaluation: sums of atomics in the default mode)
        np.testing.assert_allclose(tabs[0][k], tabs[1][k], rtol=1e-12, atol=0, equal_nan=True, err_msg=k)
