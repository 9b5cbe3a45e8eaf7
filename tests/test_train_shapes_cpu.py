"""The cases of test_train_shapes_gpu.py without a GPU: the product's rule headers, compiled into the serial driver (tests/emul),
against the oracle per sequence at band widths other than the golden models' -- the reference schedule (linear 0) and the merged
sweep on the shadow automaton (linear 2), generic and table-driven forms, pruned and complete lists -- at the sizes a serial
driver can take (L <= 300, no 200- or 1100-sequence groups); the counts of unskipped sequences that the GPU cases assert, from
the oracle alone (so the inputs are verified here); and a self-test of the checker: the error the batch gradient hides and the
per-sequence rows catch."""
import numpy as np
import pytest

from oracle import pyoracle as po
from tests import train_check as tc
from tests.emul.pyemul import Emul
from tests.test_emul_vs_oracle import PAR as PAR_TEXT
from tests.test_pair_posterior_gpu import perturbed
from tests.test_train_shapes_gpu import (B_GRID, C_PATTERNS, F_MODELS, P1, WINDOWS, assert_unskipped, edge_case_batch, forms_batch,
                                         all_skipped_batch, maker, model_batch, n_base_batch, ranged_batch, streamed_batch,
                                         three_slot_batch, width_batch)
from tests.util import assert_log_close, gpath

L_MAX = 300
MODES = [(linear, fast, prune) for linear in (0, 2) for fast in (0, 1) for prune in (0, 1)]


class _X:
    """initial_params through the oracle (perturbed() needs only that)"""

    def __init__(self, o):
        self.o = o

    def initial_params(self, lam):
        x = self.o.get_params()
        x[-2:] = lam
        return x


def x_of(pattern, W, C):
    return perturbed(_X(po.make_oracle(pattern, W, C, min_bpp=1e-4, tau=0.1)))


def emul_against_oracle(e, x, refs, seqs, quals, l_max=L_MAX, modes=MODES):
    """Emul.train_seq in every mode against the oracle's rows, at the CPU driver's bound (test_round4_cpu.py): rtol 1e-9,
    atol 1e-11.  The merged sweep needs a shadow state and a finite Z(nasi); the driver refuses a sequence the oracle skips."""
    n = 0
    for linear, fast, prune in modes:
        e.set_prune(prune)
        mask = e.set_fast(fast)
        if linear == 2 and not mask & 8:
            continue
        for k, (s, q) in enumerate(zip(seqs, quals)):
            if len(s) > l_max:
                continue
            a, w = refs.seq[k], "%s, linear %d fast %d prune %d" % (tc.where_of(k, seqs, quals), linear, fast, prune)
            b = e.train_seq(x, s, q, linear=linear)
            for name in ("Zo", "Zari", "Znasi"):
                assert_log_close(b[name], a[name], rtol=1e-11, what="%s: %s" % (w, name))
            if a["skipped"] or (linear == 2 and not np.isfinite(a["Znasi"])):
                assert b["skipped"] == 2, w
                continue
            assert b["skipped"] == 0, w
            assert b["f"] == pytest.approx(a["f"], rel=1e-10, abs=1e-12), w
            tc.compare_counts(b, a, w, rtol=1e-9, atol=1e-11, track=False)
            n += 1
    return n


@pytest.mark.parametrize("W,C", B_GRID)
def test_band_widths(W, C):
    seqs, quals = width_batch(W, C)
    x = x_of(P1, W, C)
    refs = tc.oracle_train_refs(maker(P1, W, C, x), seqs, quals)
    n = len(seqs) // 2 - 3
    assert all(refs.seq[k]["skipped"] and refs.seq[k]["Zari"] == -np.inf for k in range(6))
    assert_unskipped(refs, quals, exactly=(n, n))
    # (the serial driver's time goes with L W^2: above W = 50 the sequences up to L = W only, in what the GPU runs by default --
    # the merged sweep with the table-driven forms and pruned lists -- and up to W = 100 in the reference schedule with the generic
    # rules as well)
    l_max, modes = (L_MAX, MODES) if W <= 50 else (W, [(0, 0, 0), (2, 1, 1)]) if W <= 100 else (W, [(2, 1, 1)])
    assert emul_against_oracle(Emul(P1, PAR_TEXT, W, C, 1e-4, 0.1, 0), x, refs, seqs, quals, l_max, modes) >= len(modes) * 4


@pytest.mark.parametrize("pattern", [P1] + list(C_PATTERNS))
def test_patterns(pattern):
    seqs, quals = forms_batch()
    x = x_of(pattern, 50, 30)
    refs = tc.oracle_train_refs(maker(pattern, 50, 30, x), seqs, quals)
    n = C_PATTERNS.get(pattern, 7)
    assert_unskipped(refs, quals, exactly=(n, n))
    assert emul_against_oracle(Emul(pattern, PAR_TEXT, 50, 30, 1e-4, 0.1, 0), x, refs, seqs, quals, 200) >= 4 * 2 * (n - 2)


@pytest.mark.parametrize("model", F_MODELS)
def test_models(model):
    seqs, quals = model_batch(model)
    md = po.read_model(gpath(model))
    refs = tc.oracle_train_refs(lambda: po.oracle_from_model(gpath(model))[0], seqs, quals)
    got = refs.unskipped(quals)
    assert got[0] == got[1] >= 4, got
    if md["no_rss"]:
        return              # (the driver has no --no-rss mode: the GPU case stands on the oracle alone)
    x = po.oracle_from_model(gpath(model))[1]
    flags = (2 if md["no_prf"] else 0) | (4 if md["no_ene"] else 0) | (8 if md["softmax"] else 0)
    e = Emul(md["pattern"], po.energy_param_text(md["ene_param"]), md["max_span"], md["max_iloop"], md["min_bpp"], md["tau"], flags)
    assert emul_against_oracle(e, x, refs, seqs, quals) >= 4 * 8


@pytest.mark.parametrize("pattern", ["(.........)", P1])
def test_edge_sequences(pattern):
    seqs, quals = edge_case_batch()
    x = x_of(pattern, 50, 30)
    refs = tc.oracle_train_refs(maker(pattern, 50, 30, x), seqs, quals)
    live = [k for k in range(len(seqs)) if not refs.seq[k]["skipped"]]
    assert live == sorted([0, 1, 6, 7, 12, 13] + ([] if pattern == "(.........)" else [2, 3])), live
    emul_against_oracle(Emul(pattern, PAR_TEXT, 50, 30, 1e-4, 0.1, 0), x, refs, seqs, quals)


def test_inputs_of_the_other_gpu_cases():
    """the counts of unskipped sequences the GPU cases D, G, H and I assert, from the oracle alone"""
    x = x_of(P1, 50, 30)
    for make_batch in (three_slot_batch, streamed_batch, ranged_batch):
        seqs, quals = make_batch()
        assert_unskipped(tc.oracle_train_refs(maker(P1, 50, 30, x), seqs, quals), quals, at_least=0.9)
    seqs, quals = ranged_batch()
    assert len(seqs) == 32 and sum(c for _, c in WINDOWS) - 1 == 32 and all(f + c <= 32 for f, c in WINDOWS)
    seqs, quals = n_base_batch()
    assert_unskipped(tc.oracle_train_refs(maker(P1, 50, 30, x), seqs, quals), quals, exactly=(5, 5))
    seqs, quals = all_skipped_batch()
    x9 = x_of("(.........)", 50, 30)
    assert_unskipped(tc.oracle_train_refs(maker("(.........)", 50, 30, x9), seqs, quals), quals, exactly=(0, 0))


def test_checker_sees_what_the_batch_gradient_hides():
    """An all-positive batch (what bench.py runs); the "has motif" sweep A of one sequence wrong by a factor 1 + 1e-6.  Under
    schedule 1 k4_combine forms ENo = pa A + pn B and ENx = A (pa = Z(ari) / Z, pn = Z(nasi) / Z), so gr = pn (B - A) moves by
    pn A 1e-6 with pn of the order 1e-3 or less: the batch gradient at the suite's rtol 1e-7 / atol 1e-7 still passes, the per-sequence
    count comparison fails and names the sequence."""
    seqs, quals = forms_batch()
    seqs, quals = seqs[::2], quals[::2]
    assert all(tc.has_motif(q) for q in quals)
    x = x_of(P1, 50, 30)
    refs = tc.oracle_train_refs(maker(P1, 50, 30, x), seqs, quals)
    assert_unskipped(refs, quals, exactly=(len(seqs), 0))
    k = 4                                              # (L = 200)
    a = refs.seq[k]
    pa, pn = np.exp(a["Zari"] - a["Zo"]), np.exp(a["Znasi"] - a["Zo"])
    assert pn < 1e-2 and pa + pn == pytest.approx(1.0, rel=1e-9), (pa, pn)
    bad = {}
    for o_key, x_key in (("ENo", "ENx"), ("EHo", "EHx")):
        A = a[x_key]
        B = (a[o_key] - pa * A) / pn
        A_bad = A * (1 + 1e-6)
        bad[o_key], bad[x_key] = pa * A_bad + pn * B, A_bad
    gr_ref = refs.batch[1]
    gr_bad = gr_ref.copy()
    gr_bad[:-2] += (bad["ENo"] - bad["ENx"]) - (a["ENo"] - a["ENx"])
    gr_bad[-2:] += (bad["EHo"] - bad["EHx"]) - (a["EHo"] - a["EHx"])
    assert np.abs(gr_bad - gr_ref).max() > 0
    np.testing.assert_allclose(gr_bad, gr_ref, **tc.GR_TOL)               # the hole: invisible to the batch gradient
    nt = len(a["ENo"])
    counts = {key: np.array([bad[key] if j == k else r[key] for j, r in enumerate(refs.seq)]) for key in tc.COUNTS}
    stats = np.array([[r["Zo"], r["Zari"], r["Znasi"], r["f"], r["skipped"]] for r in refs.seq])
    with pytest.raises(AssertionError, match=r"sequence 4 \(L 200, with motif\): EN[ox]\[\d+\]"):
        tc.check_rows(stats, counts, refs, seqs, quals)
    counts[tc.COUNTS[0]][k] = a["ENo"]
    counts["ENx"][k], counts["EHo"][k], counts["EHx"][k] = a["ENx"], a["EHo"], a["EHx"]
    tc.check_rows(stats, counts, refs, seqs, quals)                       # (and the unperturbed rows pass)
    assert nt == len(x) - 2
