"""Base-pair posteriors under the motif model on the GPU: the scaled-linear reduction (k4_pairs), the
log-space form of the fused scan kernel, the compaction into one list in (sequence, i, j) order, streamed batches and
`scan --out-pairs`, against the oracle's inside / outside tables of the scan's first sum pass (motif_scanner.hpp:186-192)."""
import re

import numpy as np
import pytest

from oracle import pyoracle as po
from rnaelem_amd import api, cli, io, synth
from tests.pair_check import check_against_oracle
from tests.util import gpath

pytestmark = pytest.mark.gpu

PAR = "~T2004~"
PATTERNS = ["((.*.))", "(.....)", "(.(.).)", "(((((.*.)))))(((.*.)))"]


def ragged_batch():
    """lengths 13 .. 200 at max_span 50 (13 and 40 have L <= W); a final quality of 5 on every other sequence"""
    seqs, quals = [], []
    for L in (13, 40, 97, 131, 200):
        s, q = synth.synth_batch(1, L, seed=900 + L)
        seqs += s
        quals += q
    for k in range(0, len(quals), 2):
        quals[k][-1] = 5
    return seqs, quals


def perturbed(eng, lam=0.7):
    x = eng.initial_params(lam)
    x[:-2] += np.linspace(-0.3, 0.3, len(x) - 2)
    x[-1] += 0.2
    return x


@pytest.mark.parametrize("pattern", PATTERNS)
def test_pair_posteriors_match_the_oracle(pattern):
    seqs, quals = ragged_batch()
    eng = api.Engine(pattern, PAR, 50, 30, 1e-4, 0.1, 0, 0)
    eng.load_batch(seqs, quals)
    x = perturbed(eng)
    o = po.make_oracle(pattern, 50, 30, min_bpp=1e-4, tau=0.1)
    o.set_params(x)
    check_against_oracle(eng, o, seqs, quals, x)
    assert eng.last_timing()[2] == 0 and eng.last_timing()[0] >= eng.last_timing()[1] > 0


def test_log_space_form_for_sequences_out_of_the_double_range():
    """lambda = 40: Z leaves the double range of the scaled-linear tables; those sequences go through the fused scan kernel's
    first pass in log space and the same rule"""
    recs = io.read_fastq(gpath("syn_L150_n8.fq"))
    seqs, quals = [s for _, s, _ in recs], [q for _, _, q in recs]
    eng = api.Engine("((.*.))", PAR, 50, 30, 1e-4, 0.1, 0, 0)
    eng.load_batch(seqs, quals)
    x = eng.initial_params(40.0)
    o = po.make_oracle("((.*.))", 50, 30, min_bpp=1e-4, tau=0.1)
    o.set_params(x)
    check_against_oracle(eng, o, seqs, quals, x)
    assert eng.last_timing()[2] > 0


def test_log_space_pipeline_option():
    seqs, quals = ragged_batch()
    eng = api.Engine("((.*.))", PAR, 50, 30, 1e-4, 0.1, 0, 0)
    eng.set_option("pipeline", 3)
    eng.load_batch(seqs, quals)
    x = perturbed(eng)
    o = po.make_oracle("((.*.))", 50, 30, min_bpp=1e-4, tau=0.1)
    o.set_params(x)
    check_against_oracle(eng, o, seqs, quals, x)


def same(a, b):
    """The same pairs (cells, in order) and the same values.  The pair stages sum in a fixed order, but the tables they read come
    from the scan's sum passes, whose heavy sums gather through LDS atomics: a repeat agrees to the last bits, not bit for bit."""
    assert len(a) == len(b)
    for (ia, ja, pa, ua), (ib, jb, pb, ub) in zip(a, b):
        assert np.array_equal(ia, ib) and np.array_equal(ja, jb)
        np.testing.assert_allclose(pb, pa, rtol=1e-13, atol=1e-300)
        np.testing.assert_allclose(ub, ua, rtol=1e-13, atol=1e-15)


def test_invariants_threshold_repeats_and_no_rss():
    seqs, quals = ragged_batch()
    eng = api.Engine("(.(.).)", PAR, 50, 30, 1e-4, 0.1, 0, 0)
    eng.load_batch(seqs, quals)
    x = perturbed(eng)
    full = eng.pair_posteriors(x, 0.0)
    for (ii, jj, pp, unp), seq in zip(full, seqs):
        L = len(seq)
        assert np.all(unp >= -1e-12) and np.all(unp <= 1.0)
        per_base = np.zeros(L)
        np.add.at(per_base, ii, pp)
        np.add.at(per_base, jj - 1, pp)
        assert np.all(per_base <= 1.0 + 1e-12)
        assert np.all(pp >= 0.0)
    cut = eng.pair_posteriors(x, 1e-3)
    for (ii, jj, pp, unp), (ci, cj, cp, cu) in zip(full, cut):
        keep = pp >= 1e-3
        assert np.array_equal(ci, ii[keep]) and np.array_equal(cj, jj[keep])
        np.testing.assert_allclose(cp, pp[keep], rtol=1e-13, atol=1e-300)
        np.testing.assert_allclose(cu, unp, rtol=1e-13, atol=1e-15)
    same(eng.pair_posteriors(x, 0.0), full)

    m = io.read_model(gpath("2.model"))
    assert m["no_rss"]
    e2 = io.engine_from_model(m)
    e2.load_batch(seqs, quals)
    for ii, jj, pp, unp in e2.pair_posteriors(m["x"], 0.0):
        assert len(pp) == 0 and np.all(unp == 1.0)


def test_streamed_batch_equals_the_resident_one():
    seqs, quals = synth.synth_batch(20, 90, seed=77)
    seqs = [s[: 40 + 3 * k] for k, s in enumerate(seqs)]
    quals = [q[: 41 + 3 * k] for k, q in enumerate(quals)]
    for k in range(0, 20, 3):
        quals[k][-1] = 5
    res = {}
    for mr in (0, 7):
        eng = api.Engine("((.*.))", PAR, 50, 30, 1e-4, 0.1, 0, 0)
        if mr:
            eng.set_option("max_resident", mr)
        eng.load_batch(seqs, quals)
        res[mr] = eng.pair_posteriors(perturbed(eng), 0.0)
    same(res[7], res[0])
    assert sum(len(r[2]) for r in res[0]) > 0


def test_pair_posteriors_change_nothing_else():
    """scan, pair_posteriors, scan, train_eval on one handle give what a scan and a train evaluation give on a fresh handle"""
    seqs, quals = ragged_batch()
    out = {}
    for with_pairs in (False, True):
        eng = api.Engine("((.*.))", PAR, 50, 30, 1e-4, 0.1, 0, 0)
        eng.set_option("deterministic", 1)
        eng.load_batch(seqs, quals)
        x = perturbed(eng)
        if with_pairs:
            eng.scan(x)
            eng.pair_posteriors(x, 0.0)
        out[with_pairs] = eng.scan(x), eng.train_eval(x)
    (ra, ea), ta = out[False]
    (rb, eb), tb = out[True]
    np.testing.assert_allclose(eb, ea, rtol=1e-13, atol=1e-300)
    for p, q in zip(ra, rb):     # (the scan's posteriors are summed with atomics: equal to the last bits)
        assert (p["Ys"], p["Ye"], p["rss"]) == (q["Ys"], q["Ye"], q["rss"]) and np.array_equal(p["psihat"], q["psihat"])
        assert q["exist_prob"] == pytest.approx(p["exist_prob"], rel=1e-13)
        for key in ("start", "inner", "end"):
            assert np.array_equal(np.isfinite(p[key]), np.isfinite(q[key])), key
            np.testing.assert_allclose(q[key], p[key], rtol=1e-13, atol=1e-13, err_msg=key)
    assert ta[0] == tb[0] and np.array_equal(ta[1], tb[1]) and ta[2:] == tb[2:]     # (deterministic train evaluation: bits)


NUMBER = re.compile(r"-?(?:inf|nan|\d+(?:\.\d*)?(?:e[-+]\d+)?)")


def same_scan_text(a, b):
    """Byte-identical up to the last bits of the scan's posteriors, which are summed with atomics: a log posterior within 1e-15 of
    0 (a position the motif takes for certain) prints its own rounding noise, e.g. -3.31549e-15 in one run and -3.35549e-15 in
    the next.  Everything else -- layout, ids, parses, regions -- is compared as text."""
    assert NUMBER.sub("#", a) == NUMBER.sub("#", b)
    na, nb = NUMBER.findall(a), NUMBER.findall(b)
    assert len(na) == len(nb)
    diff = [(u, v) for u, v in zip(na, nb) if u != v]
    for u, v in diff:
        assert abs(float(u) - float(v)) <= 1e-12 + 1e-5 * abs(float(v)), (u, v)
    assert len(diff) <= 5, diff


def test_command_line_writes_the_pair_file(tmp_path):
    fq, model = gpath("positive_head6.fq"), gpath("trna_a.model")
    a0, a1, pf = str(tmp_path / "a0.raw"), str(tmp_path / "a.raw"), str(tmp_path / "p.txt")
    cli.main(["scan", "-f", fq, "-q", model, "--out1", a0])
    cli.main(["scan", "-f", fq, "-q", model, "--out1", a1, "--out-pairs", pf])
    same_scan_text(open(a1).read(), open(a0).read())
    m = io.read_model(model)
    recs = io.read_fastq(fq)
    eng = io.engine_from_model(m)
    eng.load_batch([s for _, s, _ in recs], [q for _, _, q in recs])
    want = eng.pair_posteriors(m["x"], 1e-3)
    got = io.read_pair_records(pf)
    assert [g[0] for g in got] == [r[0] for r in recs]
    assert sum(len(g[2]) for g in got) > 0
    for (rid, unp, prs), (ii, jj, pp, wu) in zip(got, want):
        assert [(a, b) for a, b, _ in prs] == list(zip(ii + 1, jj))
        assert [v for _, _, v in prs] == [float("%.6g" % v) for v in pp]
        assert list(unp) == [float("%.6g" % v) for v in wu]
