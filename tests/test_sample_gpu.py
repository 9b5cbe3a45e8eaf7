"""Stochastic samples of derivations on the GPU: the inside-only sweep (launch_lin_scan_group,
SCAN_PASS_INSIDE) and k_sample, against the oracle's posteriors, the CPU driver of the same rule, other forms and runs of the same draws, and
`scan --out-samples`."""
import numpy as np
import pytest

from oracle import pyoracle as po
from rnaelem_amd import api, cli, io, synth
from tests.pair_check import oracle_pairs, oracle_refs
from tests.sample_check import Driver, check_distribution, check_valid
from tests.test_pair_posterior_gpu import PAR, PATTERNS, perturbed, ragged_batch, same_scan_text
from tests.util import gpath

pytestmark = pytest.mark.gpu

N = 4000


def engine(pattern, **opts):
    eng = api.Engine(pattern, PAR, 50, 30, 1e-4, 0.1, 0, 0)
    for k, v in opts.items():
        eng.set_option(k, v)
    return eng


def agree(a, b, what, frac=0.999):
    """the same draws: at least frac of the samples are the same derivation (a last-bit difference of the tables can flip one)"""
    assert len(a) == len(b)
    tot = same = 0
    for (ra, na, la, sa), (rb, nb, lb, sb) in zip(a, b):
        assert sa == sb, what
        for x, y, u, v in zip(ra, rb, na, nb):
            tot += 1
            same += x == y and np.array_equal(u, v)
    assert same >= frac * tot, (what, same, tot)
    return same, tot


@pytest.mark.parametrize("pattern", PATTERNS)
def test_every_sample_is_a_valid_derivation(pattern):
    seqs, quals = ragged_batch()
    eng = engine(pattern)
    eng.load_batch(seqs, quals)
    x = perturbed(eng)
    names = eng.describe()["node"]
    res = eng.sample_structures(x, 300, seed=1)
    assert eng.last_timing()[2] == 0 and eng.last_timing()[0] > 0
    for k, (rss, nodes, logp, st) in enumerate(res):
        assert st == eng.SAMPLED, k
        assert np.all(np.isfinite(logp)) and np.all(logp <= 1e-12)
        check_valid(rss, nodes, eng.pairs(k)[0], min(len(seqs[k]), 50), len(names), names, what=(pattern, k))
        seen = {}
        for r, h, lp in zip(rss, nodes, logp):     # the same (rss, nodes): the same derivation, the same log-probability
            key = (r, h.tobytes())
            if key in seen:
                assert lp == pytest.approx(seen[key], rel=1e-12, abs=1e-12)
            seen[key] = lp


@pytest.mark.parametrize("pattern", ["((.*.))", "(.....)"])
def test_sample_frequencies_match_the_oracle(pattern):
    seqs, quals = ragged_batch()
    eng = engine(pattern)
    eng.load_batch(seqs, quals)
    x = perturbed(eng)
    M = len(eng.describe()["node"])

    def make():
        o = po.make_oracle(pattern, 50, 30, min_bpp=1e-4, tau=0.1)
        o.set_params(x)
        return o

    refs = oracle_refs(make, seqs, quals)
    res = eng.sample_structures(x, N, seed=3)
    for k, ((rss, nodes, logp, st), ref) in enumerate(zip(res, refs)):
        assert st == eng.SAMPLED and ref["P"] is not None, k
        check_distribution(rss, nodes, ref["P"], ref["scan"], M, what=(pattern, k))
        # derivations drawn often: their frequency against exp(logp)
        count, lps, checked = {}, {}, 0
        for r, h, lp in zip(rss, nodes, logp):
            key = (r, h.tobytes())
            count[key] = count.get(key, 0) + 1
            lps[key] = lp
        for key, c in count.items():
            if c >= 50:
                p = np.exp(lps[key])
                assert abs(c / N - p) <= 5 * np.sqrt(p * (1 - p) / N) + 2e-3, (pattern, k, c / N, p)
                checked += 1
        if len(seqs[k]) <= 40:   # (short sequences: some derivations are drawn often)
            assert checked > 0, (pattern, k)


def test_forms_and_runs_draw_the_same_samples():
    seqs, quals = ragged_batch()
    eng = engine("((.*.))")
    eng.load_batch(seqs, quals)
    x = perturbed(eng)
    full = eng.sample_structures(x, 400, seed=9)
    agree(eng.sample_structures(x, 400, seed=9), full, "repeat")
    drv = Driver("((.*.))", PAR)
    cpu = []
    for k, (s, q) in enumerate(zip(seqs, quals)):
        rss, nodes, logp, st = drv.sample(x, s, q, 400, 9, k)
        cpu.append((rss, nodes, logp, st))
    agree(cpu, full, "CPU driver")
    # two halves with their batch offsets as index_base
    h0, h1 = engine("((.*.))"), engine("((.*.))")
    h0.load_batch(seqs[:2], quals[:2])
    h1.load_batch(seqs[2:], quals[2:])
    agree(h0.sample_structures(x, 400, seed=9) + h1.sample_structures(x, 400, seed=9, index_base=2), full, "halves")
    other = eng.sample_structures(x, 400, seed=10)
    assert sum(a[0] != b[0] for a, b in zip(other, full)) > 0


def test_streamed_batch_draws_what_the_resident_one_draws():
    seqs, quals = synth.synth_batch(20, 90, seed=77)
    seqs = [s[: 40 + 3 * k] for k, s in enumerate(seqs)]
    quals = [q[: 41 + 3 * k] for k, q in enumerate(quals)]
    res = {}
    for mr in (0, 7):
        eng = engine("((.*.))", **({"max_resident": mr} if mr else {}))
        eng.load_batch(seqs, quals)
        res[mr] = eng.sample_structures(perturbed(eng), 200, seed=5)
    agree(res[7], res[0], "streamed")


def test_log_space_form_for_sequences_out_of_the_double_range():
    """lambda = 40: Z leaves the double range of the scaled-linear tables; those sequences are sampled on the fused scan kernel's
    log tables, with the same rule"""
    recs = io.read_fastq(gpath("syn_L150_n8.fq"))
    seqs, quals = [s for _, s, _ in recs], [q for _, _, q in recs]
    eng = engine("((.*.))")
    eng.load_batch(seqs, quals)
    x = eng.initial_params(40.0)
    M = len(eng.describe()["node"])
    res = eng.sample_structures(x, N, seed=2)
    assert eng.last_timing()[2] > 0

    def make():
        o = po.make_oracle("((.*.))", 50, 30, min_bpp=1e-4, tau=0.1)
        o.set_params(x)
        return o

    refs = oracle_refs(make, seqs, quals)
    names = eng.describe()["node"]
    for k, ((rss, nodes, logp, st), ref) in enumerate(zip(res, refs)):
        if ref["P"] is None:
            assert st == eng.NO_PARSE, k
            continue
        assert st == eng.SAMPLED and np.all(np.isfinite(logp)), k
        check_valid(rss[:200], nodes[:200], eng.pairs(k)[0], min(len(seqs[k]), 50), M, names, what=("lambda 40", k))
        check_distribution(rss, nodes, ref["P"], ref["scan"], M, what=("lambda 40", k))


def test_log_space_pipeline_option_draws_the_same_samples():
    seqs, quals = ragged_batch()
    e3, e4 = engine("((.*.))", pipeline=3), engine("((.*.))")
    e3.load_batch(seqs, quals)
    e4.load_batch(seqs, quals)
    x = perturbed(e4)
    a3 = e3.sample_structures(x, 400, seed=9)
    assert all(st == e3.SAMPLED for _, _, _, st in a3)
    agree(a3, e4.sample_structures(x, 400, seed=9), "pipeline 3")
    for (_, _, la, _), (_, _, lb, _) in zip(a3, e4.sample_structures(x, 400, seed=9)):
        assert np.all(np.isfinite(la))
    with pytest.raises(api.ElemdpError):
        e3.sample_structures(x, 0)


def test_sampling_changes_nothing_else():
    seqs, quals = ragged_batch()
    out = {}
    for with_samples in (False, True):
        eng = engine("((.*.))", deterministic=1)
        eng.load_batch(seqs, quals)
        x = perturbed(eng)
        if with_samples:
            eng.sample_structures(x, 50)
        out[with_samples] = eng.scan(x), eng.pair_posteriors(x, 0.0), eng.train_eval(x)
    (ra, _), pa, ta = out[False]
    (rb, _), pb, tb = out[True]
    for p, q in zip(ra, rb):
        assert (p["Ys"], p["Ye"], p["rss"]) == (q["Ys"], q["Ye"], q["rss"]) and np.array_equal(p["psihat"], q["psihat"])
        for key in ("start", "inner", "end"):
            np.testing.assert_allclose(q[key], p[key], rtol=1e-13, atol=1e-13, err_msg=key)
    for (ia, ja, xa, ua), (ib, jb, xb, ub) in zip(pa, pb):
        assert np.array_equal(ia, ib) and np.array_equal(ja, jb)
        np.testing.assert_allclose(xb, xa, rtol=1e-13, atol=1e-300)
    assert ta[0] == tb[0] and np.array_equal(ta[1], tb[1]) and ta[2:] == tb[2:]


@pytest.mark.parametrize("with_mea", [False, True])
def test_command_line_writes_the_sample_file(tmp_path, with_mea):
    fq, model = gpath("positive_head6.fq"), gpath("trna_a.model")
    a0, a1, sf = str(tmp_path / "a0.raw"), str(tmp_path / "a.raw"), str(tmp_path / "s.txt")
    cli.main(["scan", "-f", fq, "-q", model, "--out1", a0])
    extra = ["--out-mea", str(tmp_path / "m.txt")] if with_mea else []
    cli.main(["scan", "-f", fq, "-q", model, "--out1", a1, "--out-samples", sf, "--n-samples", "30"] + extra)
    same_scan_text(open(a1).read(), open(a0).read())
    recs = io.read_fastq(fq)
    got = io.read_sample_records(sf)
    assert [g[0] for g in got] == [r[0] for r in recs]
    m = io.read_model(model)
    eng = io.engine_from_model(m)
    eng.load_batch([s for _, s, _ in recs], [q for _, _, q in recs])
    want = eng.sample_structures(m["x"], 30, 0)
    for (rid, status, rows), (rss, nodes, logp, st) in zip(got, want):
        assert status == "sampled"
        assert len(rows) == 30 and st == eng.SAMPLED
        # (the same draws; a log-probability agrees to the last bits of the tables, which are summed with LDS atomics)
        assert sum(r[5] == t for r, t in zip(rows, rss)) >= 29
        np.testing.assert_allclose([r[1] for r in rows if r[5] in rss], [v for v, t in zip(logp, rss) if t in [r[5] for r in rows]],
                                   rtol=1e-12)
