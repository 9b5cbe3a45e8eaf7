"""The usefulness mask of the train sweeps on the GPU: the mask the plan kernel builds against the host
entry (same rule functions, plan_rules.h); train_eval and seq_counts with option useful_mask 1 against 0 -- equal bit for bit in
the deterministic mode (the dropped terms are exact zeros), within the tolerances of tests/test_gpu_parity.py against the oracle
(fn 1e-10, gr rtol 1e-8 / atol 1e-10) in the default mode, whose atomic adds arrive in any order -- over ragged and uniform
batches, both patterns, max_iloop 5, lambda (0, 0) and (1, 1), a ranged and a streamed evaluation; the per-sequence rows against
the oracle with the mask on; a batch under a structure constraint, whose unpaired flags are not all ones; the mask of all ones
that a sequence too large for the plan kernel's LDS gets; and the scan records and debug_tables, which do not see the mask, with
the option 1 and 0 once a train evaluation has built the mask.
Everything runs under the NaN poisoning that tests/conftest.py turns on: a read of an entry that the masked sweeps left unstored
would show as NaN."""
import numpy as np
import pytest

from rnaelem_amd import api, io
from tests import train_check as tc
from tests.test_pair_posterior_gpu import perturbed
from tests.test_pair_shapes_gpu import batch, oracle_maker
from tests.test_useful_mask_cpu import FIX_CASES, fix_inputs
from tests.util import gpath

pytestmark = pytest.mark.gpu

PAR = "~T2004~"
P1, P5 = "((.*.))", "(.....)"


def ragged_batch():
    """40 sequences, L from 20 to 120 (not sorted), every third with N bases, one poly-A (no kept pair), both labels"""
    rng = np.random.default_rng(40)
    lens = [int(v) for v in rng.permutation(np.linspace(20, 120, 39).astype(int))]
    seqs, quals = batch(lens, seed=40)
    seqs.insert(17, np.full(50, 1, dtype=np.uint8))
    quals.insert(17, np.append(np.full(50, 10, dtype=np.uint8), np.uint8(0)))
    return seqs, quals


def l150_batch():
    recs = io.read_fastq(gpath("syn_L150_n8.fq"))
    return [np.asarray(s, dtype=np.uint8) for _, s, _ in recs], [np.asarray(q, dtype=np.uint8) for _, _, q in recs]


def engine(pattern=P1, C=30, opts=()):
    eng = api.Engine(pattern, PAR, 50, C, 1e-4, 0.1, 0, 0)
    for k, v in opts:
        eng.set_option(k, v)
    return eng


def test_gpu_mask_equals_the_host_entry():
    seqs, quals = ragged_batch()
    eng = engine()
    eng.load_batch(seqs, quals)
    n_bits = 0
    for k in range(len(seqs)):
        kept = eng.pairs(k)[0]
        got, want = eng.useful_mask(k), api.useful_mask_host(kept, max_iloop=30)
        assert got.shape == want.shape == (min(len(seqs[k]), 50) + 1, len(seqs[k]) + 1)
        assert np.array_equal(got, want), "sequence %d (L %d): %d cells differ" % (k, len(seqs[k]), int((got != want).sum()))
        n_bits += int(np.count_nonzero(got))
    assert n_bits > 0 and not eng.useful_mask(17).any()        # (the poly-A sequence keeps no pair: nothing is useful)
    eng5 = engine(C=5)
    eng5.load_batch(seqs[:6], quals[:6])
    for k in range(6):
        assert np.array_equal(eng5.useful_mask(k), api.useful_mask_host(eng5.pairs(k)[0], max_iloop=5)), k


def both_ways(eng, x, rows=True):
    """(train_eval, seq_stats, seq_counts) with the mask on, then off"""
    out = []
    for on in (1, 0):
        eng.set_option("useful_mask", on)
        res = eng.train_eval(x)
        out.append((res, eng.seq_stats(), {k: v.copy() for k, v in eng.seq_counts().items()} if rows else None))
    eng.set_option("useful_mask", 1)
    return out


def compare(a, b, exact, what):
    (ra, sa, ca), (rb, sb, cb) = a, b
    print("%s: fn %.17g / %.17g  max |gr diff| %.3g" % (what, ra[0], rb[0], float(np.abs(ra[1] - rb[1]).max())))
    assert np.isfinite(ra[0]) and np.all(np.isfinite(ra[1])), what
    assert ra[2] == rb[2] and ra[3] == rb[3], what
    if exact:
        assert ra[0] == rb[0], (what, ra[0], rb[0])
        assert np.array_equal(ra[1], rb[1]), what
        assert np.array_equal(sa, sb, equal_nan=True), what
        for k in ca or ():
            assert np.array_equal(ca[k], cb[k]), (what, k)
    else:
        assert ra[0] == pytest.approx(rb[0], rel=1e-10), what
        np.testing.assert_allclose(ra[1], rb[1], rtol=1e-8, atol=1e-10, err_msg=what)
        np.testing.assert_allclose(sa, sb, rtol=1e-10, atol=1e-10, err_msg=what)
        for k in ca or ():
            np.testing.assert_allclose(ca[k], cb[k], rtol=1e-8, atol=1e-10, err_msg="%s %s" % (what, k))


CASES = {
    "ragged": (ragged_batch, P1, 30, None, (), None),
    "L150x8": (l150_batch, P1, 30, None, (), None),
    "ragged (.....)": (ragged_batch, P5, 30, None, (), None),
    "L150x8 (.....)": (l150_batch, P5, 30, None, (), None),
    "ragged max_iloop 5": (ragged_batch, P1, 5, None, (), None),
    "ragged lambda 0": (ragged_batch, P1, 30, (0.0, 0.0), (), None),
    "ragged lambda 1": (ragged_batch, P1, 30, (1.0, 1.0), (), None),
    "ragged window": (ragged_batch, P1, 30, None, (), (5, 17)),
    "ragged streamed": (ragged_batch, P1, 30, None, (("max_resident", 7),), None),
}


@pytest.mark.parametrize("name", list(CASES))
def test_mask_on_against_off(name):
    make, pattern, C, lam, opts, window = CASES[name]
    seqs, quals = make()
    eng = engine(pattern, C, opts)
    eng.load_batch(seqs, quals)
    x = perturbed(eng)
    if lam is not None:
        x[-2:] = lam
    if window is not None:
        eng.set_option("eval_first", window[0])
        eng.set_option("eval_count", window[1])
    rows = not opts
    for det in (1, 0):
        eng.set_option("deterministic", det)
        on, off = both_ways(eng, x, rows)
        compare(on, off, bool(det), "%s, deterministic %d" % (name, det))


@pytest.mark.parametrize("pattern", [P1, P5])
def test_rows_against_the_oracle_with_the_mask_on(pattern):
    """fn, gr and the rows of every sequence (seq_stats, seq_counts) against the oracle: tests/train_check.py"""
    seqs, quals = ragged_batch()
    eng = engine(pattern)
    eng.load_batch(seqs, quals)
    x = perturbed(eng)
    tc.check_train_path(eng, seqs, quals, x, oracle_maker(pattern, 50, 30, x))


def test_mask_and_train_under_a_structure_constraint():
    """Unpaired flags that are not all ones (the unp terms of the rules in k_useful_mask): the GPU-built mask equals the host
    entry's with the same flags and differs from the one without them.  The constrained evaluation runs the generic kernels,
    which take no mask: the option changes nothing there, bit for bit in the deterministic mode."""
    dbs = [db for _, db in FIX_CASES]
    seqs = [np.array([{"(": 3, ")": 2, ".": 1}[c] for c in db], dtype=np.uint8) for db in dbs]
    quals = [np.append(np.full(len(db), 10, dtype=np.uint8), np.uint8(k % 2)) for k, db in enumerate(dbs)]
    eng = api.Engine(P1, PAR, 50, 30, 1e-4, 0.1, api.DBG_FIX_RSS, 0)
    eng.load_batch(seqs, quals, fix_rss=dbs)
    for k, db in enumerate(dbs):
        kept, unp = fix_inputs(db, min(len(db), 50))
        assert np.array_equal(eng.pairs(k)[0], kept), k
        got = eng.useful_mask(k)
        assert got.any() and np.array_equal(got, api.useful_mask_host(kept, max_iloop=30, unp=unp)), k
        assert not np.array_equal(got, api.useful_mask_host(kept, max_iloop=30)), k
    x = perturbed(eng)
    for det in (1, 0):
        eng.set_option("deterministic", det)
        on, off = both_ways(eng, x)
        compare(on, off, bool(det), "structure constraint, deterministic %d" % det)


def test_sequence_too_large_for_the_plan_kernel_gets_all_ones():
    """option useful_mask_lds_kb below what the longest sequence needs: every byte of the mask is 255 (every entry useful), and the
    train evaluation is what it is without a mask"""
    seqs, quals = ragged_batch()
    eng = engine(opts=(("useful_mask_lds_kb", 1), ("deterministic", 1)))
    eng.load_batch(seqs[:8], quals[:8])
    for k in range(8):
        assert np.all(eng.useful_mask(k) == 255), k
    on, off = both_ways(eng, perturbed(eng))
    compare(on, off, True, "mask of all ones")
    with pytest.raises(api.ElemdpError):
        eng.set_option("useful_mask_lds_kb", 151)


def close_sums(a, b, what):
    """two runs of the scan kernels: the bound the project holds a repeated scan to (tests/test_mea_gpu.py: rtol 1e-13; the sums
    are atomic adds, whose order varies from run to run), the finiteness pattern exactly"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape and np.array_equal(np.isfinite(a), np.isfinite(b)), what
    fin = np.isfinite(a)
    err = float(np.max(np.abs(a[fin] - b[fin]) / np.maximum(np.abs(b[fin]), 1e-300), initial=0.0))
    print("%s: max relative difference %.3g" % (what, err))
    np.testing.assert_allclose(a[fin], b[fin], rtol=1e-13, atol=1e-13, err_msg=what)


def has_dead_and_live_cells(mask):
    dd, ii = np.meshgrid(np.arange(mask.shape[0]), np.arange(mask.shape[1]), indexing="ij")
    inside = ii + dd <= mask.shape[1] - 1
    return bool((mask[inside] == 0).any() and (mask[inside] != 0).any())


def test_scan_does_not_see_the_mask():
    """a train evaluation first, so that the plan holds a mask with dead cells; then the scan with the option 1 and 0: what is
    discrete is identical, the sums agree as two scans of one handle do"""
    seqs, quals = ragged_batch()
    eng = engine(opts=(("deterministic", 1),))
    eng.load_batch(seqs[:12], quals[:12])
    x = perturbed(eng)
    eng.train_eval(x)
    assert any(has_dead_and_live_cells(eng.useful_mask(k)) for k in range(12))
    got = []
    for on in (1, 0):
        eng.set_option("useful_mask", on)
        got.append(eng.scan(x))
    (ra, ea), (rb, eb) = got
    np.testing.assert_allclose(ea, eb, rtol=1e-13, atol=1e-300, err_msg="scan: expected counts")
    for n, (a, b) in enumerate(zip(ra, rb)):
        assert (a["Ys"], a["Ye"], a["rss"]) == (b["Ys"], b["Ye"], b["rss"]) and np.array_equal(a["psihat"], b["psihat"]), n
        assert a["exist_prob"] == pytest.approx(b["exist_prob"], rel=1e-13), n
        for k in ("start", "inner", "end"):
            close_sums(a[k], b[k], "scan: sequence %d %s" % (n, k))


def test_debug_tables_do_not_see_the_mask():
    """debug_tables repeats the evaluation of one sequence with the generic kernels, which take no mask: in the deterministic
    mode its tables and counts are identical, bit for bit, with the option 1 and 0"""
    seqs, quals = ragged_batch()
    eng = engine(opts=(("deterministic", 1),))
    eng.load_batch(seqs[3:4], quals[3:4])
    x = perturbed(eng)
    tabs = []
    for on in (1, 0):
        eng.set_option("useful_mask", on)
        eng.train_eval(x)
        tabs.append(eng.debug_tables())
    assert has_dead_and_live_cells(eng.useful_mask(0))
    for k in tabs[0]:
        a, b = tabs[0][k], tabs[1][k]
        fin = np.isfinite(a) & np.isfinite(b)
        print("debug_tables %s: max difference %.3g" % (k, float(np.max(np.abs(a[fin] - b[fin]), initial=0.0))))
    for k in tabs[0]:
        assert np.array_equal(tabs[0][k], tabs[1][k], equal_nan=True), k
