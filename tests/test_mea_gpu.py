"""Maximum expected accuracy structures under the motif model on the GPU: k_pair_mea behind k_pair_seq in
the scaled-linear group sweep and the log-space chunks, against the host mirror of the rule (bit for bit, on the call's own
pair posteriors) and against the optimum over the oracle's pair posteriors; streamed batches, invariants, `scan --out-mea`."""
import numpy as np
import pytest

from oracle import pyoracle as po
from rnaelem_amd import api, cli, io, synth
from tests.mea_mirror import expected_accuracy, mea_fold, pair_matrix, pairs_of
from tests.pair_check import check_against_mirror, oracle_pairs, unpaired_of
from tests.test_pair_posterior_gpu import PATTERNS, perturbed, ragged_batch, same, same_scan_text
from tests.util import gpath

pytestmark = pytest.mark.gpu

PAR = "~T2004~"
GAMMAS = (0.5, 1.0, 4.0)


def engine(pattern="((.*.))", **opts):
    eng = api.Engine(pattern, PAR, 50, 30, 1e-4, 0.1, 0, 0)
    for k, v in opts.items():
        eng.set_option(k, v)
    return eng


@pytest.mark.parametrize("pattern", PATTERNS)
def test_mea_is_bit_exact_against_the_mirror(pattern):
    seqs, quals = ragged_batch()
    eng = engine(pattern)
    eng.load_batch(seqs, quals)
    out = check_against_mirror(eng, seqs, perturbed(eng))
    assert eng.last_timing()[2] == 0
    assert any("(" in s for s in out[4.0][0])     # (the batch has paired structures at all)


@pytest.mark.parametrize("pattern", PATTERNS)
def test_mea_reaches_the_optimum_over_the_oracle_posteriors(pattern):
    seqs, quals = ragged_batch()
    eng = engine(pattern)
    eng.load_batch(seqs, quals)
    x = perturbed(eng)
    o = po.make_oracle(pattern, 50, 30, min_bpp=1e-4, tau=0.1)
    o.set_params(x)
    refs = [oracle_pairs(o, s, q) for s, q in zip(seqs, quals)]
    assert sum(r is not None for r in refs) >= 3
    for gamma in (1.0, 4.0):
        structs, scores, _ = eng.mea_structures(x, gamma)
        for k, (seq, P) in enumerate(zip(seqs, refs)):
            if P is None:
                continue
            L = len(seq)
            kept = eng.pairs(k)[0].astype(bool)
            P = P[:, :kept.shape[1]]
            q = unpaired_of(P, L)
            _, opt = mea_fold(P, kept, q, gamma)
            assert scores[k] == pytest.approx(opt, rel=1e-9), (gamma, k)
            assert expected_accuracy(structs[k], P, q, gamma) == pytest.approx(opt, rel=1e-9), (gamma, k)


def test_log_space_form_for_sequences_out_of_the_double_range():
    recs = io.read_fastq(gpath("syn_L150_n8.fq"))
    seqs, quals = [s for _, s, _ in recs], [q for _, _, q in recs]
    eng = engine()
    eng.load_batch(seqs, quals)
    check_against_mirror(eng, seqs, eng.initial_params(40.0))
    assert eng.last_timing()[2] > 0


def test_log_space_pipeline_option():
    seqs, quals = ragged_batch()
    eng = engine(pipeline=3)
    eng.load_batch(seqs, quals)
    check_against_mirror(eng, seqs, perturbed(eng))


def test_streamed_batch():
    seqs, quals = synth.synth_batch(20, 90, seed=77)
    seqs = [s[: 40 + 3 * k] for k, s in enumerate(seqs)]
    quals = [q[: 41 + 3 * k] for k, q in enumerate(quals)]
    for k in range(0, 20, 3):
        quals[k][-1] = 5
    res = {}
    for mr in (0, 7):
        eng = engine(**({"max_resident": mr} if mr else {}))
        eng.load_batch(seqs, quals)
        res[mr] = check_against_mirror(eng, seqs, perturbed(eng), (1.0,))[1.0]
    assert res[7][0] == res[0][0]
    np.testing.assert_allclose(res[7][1], res[0][1], rtol=1e-12, atol=0)
    same(res[7][2], res[0][2])


def test_invariants():
    seqs, quals = ragged_batch()
    eng = engine("(.(.).)")
    eng.load_batch(seqs, quals)
    x = perturbed(eng)
    part = []
    for gamma in (0.1, 0.5, 1.0, 2.0, 8.0):
        structs, scores, prs = eng.mea_structures(x, gamma, 0.0)
        pair_sum = []
        for k, (seq, s) in enumerate(zip(seqs, structs)):
            L, W = len(seq), min(len(seq), 50)
            assert len(s) == L
            cells = pairs_of(s)            # (balanced)
            kept = eng.pairs(k)[0]
            assert all(2 <= d <= W and i + d <= L and kept[i, d] for i, d in cells)
            ii, jj, pp, unp = prs[k]
            P, _ = pair_matrix(L, W, ii, jj, pp)
            pair_sum.append(sum(2.0 * P[i, d] for i, d in cells))
            assert scores[k] >= unp.sum() - 1e-12          # (never below the all-unpaired structure)
        part.append(pair_sum)
    part = np.array(part)
    assert np.all(np.diff(part, axis=0) >= -1e-12), part        # the pair part of the optimum does not decrease over gamma

    m = io.read_model(gpath("2.model"))
    assert m["no_rss"]
    e2 = io.engine_from_model(m)
    e2.load_batch(seqs, quals)
    structs, scores, prs = e2.mea_structures(m["x"], 1.0, 0.0)
    for seq, s, sc, (ii, jj, pp, unp) in zip(seqs, structs, scores, prs):
        assert s == "." * len(seq) and np.all(unp == 1.0) and sc == float(len(seq))

    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(api.ElemdpError) as ei:
            eng.mea_structures(x, bad)
        assert ei.value.code == -1


def test_pair_list_and_unpaired_equal_those_of_pair_posteriors():
    seqs, quals = ragged_batch()
    eng = engine()
    eng.load_batch(seqs, quals)
    x = perturbed(eng)
    for mp in (0.0, 1e-3):
        want = eng.pair_posteriors(x, mp)
        _, _, got = eng.mea_structures(x, 1.0, mp)
        same(got, want)


def test_mea_changes_nothing_else():
    """scan, mea, scan, train_eval on one handle give what a scan and a train evaluation give on a fresh handle"""
    seqs, quals = ragged_batch()
    out = {}
    for with_mea in (False, True):
        eng = engine(deterministic=1)
        eng.load_batch(seqs, quals)
        x = perturbed(eng)
        if with_mea:
            eng.scan(x)
            eng.mea_structures(x, 1.0)
        out[with_mea] = eng.scan(x), eng.train_eval(x)
    (ra, ea), ta = out[False]
    (rb, eb), tb = out[True]
    np.testing.assert_allclose(eb, ea, rtol=1e-13, atol=1e-300)
    for p, q in zip(ra, rb):
        assert (p["Ys"], p["Ye"], p["rss"]) == (q["Ys"], q["Ye"], q["rss"]) and np.array_equal(p["psihat"], q["psihat"])
        assert q["exist_prob"] == pytest.approx(p["exist_prob"], rel=1e-13)
        for key in ("start", "inner", "end"):
            assert np.array_equal(np.isfinite(p[key]), np.isfinite(q[key])), key
            np.testing.assert_allclose(q[key], p[key], rtol=1e-13, atol=1e-13, err_msg=key)
    assert ta[0] == tb[0] and np.array_equal(ta[1], tb[1]) and ta[2:] == tb[2:]


def test_command_line_writes_the_mea_file(tmp_path):
    fq, model = gpath("positive_head6.fq"), gpath("trna_a.model")
    a0, a1, a2 = (str(tmp_path / n) for n in ("a0.raw", "a1.raw", "a2.raw"))
    p0, p2, m1, m2 = (str(tmp_path / n) for n in ("p0.txt", "p2.txt", "m1.txt", "m2.txt"))
    cli.main(["scan", "-f", fq, "-q", model, "--out1", a0, "--out-pairs", p0])
    cli.main(["scan", "-f", fq, "-q", model, "--out1", a1, "--out-mea", m1])
    cli.main(["scan", "-f", fq, "-q", model, "--out1", a2, "--out-pairs", p2, "--out-mea", m2, "--mea-gamma", "1.0"])
    same_scan_text(open(a1).read(), open(a0).read())
    same_scan_text(open(a2).read(), open(a0).read())
    m = io.read_model(model)
    recs = io.read_fastq(fq)
    eng = io.engine_from_model(m)
    eng.load_batch([s for _, s, _ in recs], [q for _, _, q in recs])
    structs, scores, _ = eng.mea_structures(m["x"], 1.0)
    for path in (m1, m2):
        got = io.read_mea_records(path)
        assert [g[0] for g in got] == [r[0] for r in recs]
        assert [g[1] for g in got] == structs
        np.testing.assert_allclose([g[2] for g in got], scores, rtol=1e-12, atol=0)
    want, got = io.read_pair_records(p0), io.read_pair_records(p2)
    assert len(got) == len(want) == len(recs)
    for (ra, ua, pa), (rb, ub, pb) in zip(got, want):
        assert ra == rb and [c[:2] for c in pa] == [c[:2] for c in pb]
        np.testing.assert_allclose(ua, ub, rtol=0, atol=1e-12)
        np.testing.assert_allclose([c[2] for c in pa], [c[2] for c in pb], rtol=0, atol=1e-12)
