"""Motif-conditional pair posteriors on the CPU: the two references of tests/cond_check.py against each
other; the product rule through the test-only CPU driver (tests/cond_emul.cpp), both forms, plain and table-driven unary phases,
against the enumeration on the tiny cases of tests/test_ctx_cpu.py and against the oracle's tables at the lengths around W = 20;
empty worlds; the record format, the parser and the sharded writer; the symbols and the refusal without a device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from rnaelem_amd import api, cli, io, synth
from tests import cond_check as cd
from tests import ctx_check as cc
from tests.test_ctx_cpu import CASES, case_inputs
from tests.test_host_abi import have_gpu
from tests.test_pair_posterior_gpu import PAR, perturbed
from tests.util import REPO

HEADER = os.path.join(REPO, "include", "elemdp.h")
_refs = {}


def motif_heavy(x, hmm, by=3.0):
    """x with every pattern row of theta raised: a parse gains e^by per base it puts on the motif, so nearly every parse has it"""
    xx = np.array(x, dtype=np.float64)
    n0 = hmm["theta_sizes"][0]
    xx[n0:len(xx) - 2] += by
    return xx


def references(case):
    """(x, seqs, quals, enumerated worlds, table worlds) of a tiny case, computed once"""
    if case not in _refs:
        pattern, flags, min_bpp = case
        x, seqs, quals = case_inputs(case)
        o = cc.ctx_oracle(pattern, 50, 30, min_bpp=min_bpp, flags=flags)
        o.set_params(x)
        on = cc.ctx_oracle(pattern, 50, 30, min_bpp=min_bpp, flags=flags)
        on.set_params(cd.none_params(x, o.hmm()))
        enum = [cd.enumerated_worlds(o, s, q) for s, q in zip(seqs, quals)]
        tab = [cd.table_worlds(o, on, s, q) for s, q in zip(seqs, quals)]
        _refs[case] = (x, seqs, quals, enum, tab)
    return _refs[case]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%s-%d-%g" % c)
def test_the_two_references_agree(case):
    x, seqs, quals, enum, tab = references(case)
    for k, (e, t) in enumerate(zip(enum, tab)):
        assert np.isfinite(e["Zo"]) and np.isfinite(e["Znasi"]), k
        np.testing.assert_allclose(t["Pn"], e["Pn"], rtol=1e-8, atol=1e-12, err_msg=str((case, k)))
        if t["Pm"] is not None:
            np.testing.assert_allclose(t["Pm"], e["Pm"], rtol=1e-8, atol=1e-10, err_msg=str((case, k)))
        # the mixture of the enumerated worlds is the oracle's pair posterior
        np.testing.assert_allclose(e["e"] * e["Pm"] + (1.0 - e["e"]) * e["Pn"], t["P"], rtol=1e-8, atol=1e-12, err_msg=str((case, k)))


def test_the_worlds_differ_and_both_matter_in_the_tiny_cases():
    """the cases tell the worlds apart (a swap, or Z(ari, nasi) as a normaliser, cannot pass): somewhere the folds differ by a
    tenth of a pair, and exist_prob is neither 0 nor 1"""
    shifts, es = [], []
    for case in CASES:
        for e in references(case)[3]:
            shifts.append(e["shift"])
            es.append(e["e"])
    assert np.nanmax(shifts) > 0.1 and 1e-3 < min(es) and max(es) < 1.0 - 1e-3, (np.nanmax(shifts), min(es), max(es))


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%s-%d-%g" % c)
def test_product_rule_on_the_cpu_equals_both_references(case):
    pattern, flags, min_bpp = case
    x, seqs, quals, enum, tab = references(case)
    drv = cd.CondDriver(pattern, PAR, 50, 30, min_bpp, 0.1, flags)
    for fast in (False, True):
        drv.set_fast(fast)
        for k, (s, q) in enumerate(zip(seqs, quals)):
            L, W = len(s), min(len(s), 50)
            for form in (cd.CondDriver.LIN, cd.CondDriver.LOG):
                rec, used = drv.record(x, s, q, enum[k]["kept"], form)
                assert used == form, (case, k, form)
                cd.check_record(rec, enum[k], L, W, what=(case, k, form, fast, "enumerated"), enumerated=True)
                cd.check_record(rec, tab[k], L, W, what=(case, k, form, fast, "tables"))


W20_LENS = (5, 19, 20, 21, 47)


def w20_inputs(heavy):
    eng = api.Engine("((.*.))", PAR, 20, 10, 1e-4, 0.1, 0, 0)
    x = perturbed(eng)
    if heavy:
        x = motif_heavy(x, eng.describe())
    seqs, quals = [], []
    for L in W20_LENS:
        (s,), (q,) = synth.synth_batch(1, L, seed=300 + L)
        seqs.append(s)
        quals.append(q)
    return x, seqs, quals


@pytest.mark.parametrize("heavy", [False, True], ids=["perturbed", "motif-heavy"])
def test_product_rule_on_the_cpu_around_the_band_width(heavy):
    """L = 5, W-1, W, W+1, 2W+7 at W = 20, C = 10 against the oracle's tables; with the pattern rows raised the world without the
    motif is a sliver of the mixture (1 - e < 1e-3) and its P is still checked at full tolerance"""
    x, seqs, quals = w20_inputs(heavy)
    o = cc.ctx_oracle("((.*.))", 20, 10)
    o.set_params(x)
    on = cc.ctx_oracle("((.*.))", 20, 10)
    on.set_params(cd.none_params(x, o.hmm()))
    refs = [cd.table_worlds(o, on, s, q) for s, q in zip(seqs, quals)]
    parsable = [r for r in refs if np.isfinite(r["Zo"])]
    assert len(parsable) >= 4 and 2 * sum(r["e"] >= cd.E_MIN for r in parsable) >= len(parsable)
    if heavy:
        assert any(0.0 < 1.0 - r["e"] < 1e-3 for r in refs), [r["e"] for r in refs]
    drv = cd.CondDriver("((.*.))", PAR, 20, 10, 1e-4, 0.1, 0)
    for fast in (False, True):
        drv.set_fast(fast)
        for k, (s, q) in enumerate(zip(seqs, quals)):
            for form in (cd.CondDriver.LIN, cd.CondDriver.LOG):
                rec, used = drv.record(x, s, q, refs[k]["kept"], form)
                assert used == form
                cd.check_record(rec, refs[k], len(s), min(len(s), 20), what=(heavy, k, form, fast))


def test_empty_worlds_follow_the_conventions():
    """theta(A) = -inf: poly-A has no parse at all -- both worlds empty, exist_prob 0, shift NaN; every pattern row at -inf: no
    parse with the motif -- P_motif = 0 exactly, exist_prob 0.0, and P_none is the oracle's pair posterior of the mixture"""
    pattern = "((.*.))"
    o = cc.ctx_oracle(pattern)
    x0 = perturbed(api.Engine(pattern, PAR, 50, 30, 1e-4, 0.1, 0, 0))
    x, seqs, quals = cc.no_parse_inputs(x0, o.hmm())
    o.set_params(x)
    on = cc.ctx_oracle(pattern)
    on.set_params(cd.none_params(x, o.hmm()))
    drv = cd.CondDriver(pattern, PAR)
    for form in (cd.CondDriver.LIN, cd.CondDriver.LOG):
        for k in (0, 1):
            ref = cd.table_worlds(o, on, seqs[k], quals[k])
            assert np.isfinite(ref["Zo"]) == (k == 1)
            rec, used = drv.record(x, seqs[k], quals[k], ref["kept"], form)
            assert used == form          # (an empty world is no range failure)
            cd.check_record(rec, ref, len(seqs[k]), min(len(seqs[k]), 50), what=(form, k))
            if k == 0:
                assert rec["exist_prob"] == 0.0 and np.isnan(rec["shift"]) and np.all(rec["p_none"] == 0.0)
    xn = cd.none_params(x0, o.hmm())
    on.set_params(xn)
    (s,), (q,) = synth.synth_batch(1, 40, seed=11)
    ref = cd.table_worlds(on, on, s, q)
    assert not np.isfinite(ref["Zari"]) and ref["Pn"].max() > 0.1
    for form in (cd.CondDriver.LIN, cd.CondDriver.LOG):
        rec, _ = drv.record(xn, s, q, ref["kept"], form)
        cd.check_record(rec, ref, 40, 40, what=("no motif", form))
        assert rec["exist_prob"] == 0.0 and np.all(rec["p_motif"] == 0.0) and np.isnan(rec["shift"])
        np.testing.assert_allclose(rec["p_none"], ref["P"][rec["i"], rec["j"] - rec["i"]], rtol=1e-8, atol=1e-12)


def test_a_model_without_structure_has_no_pairs():
    m = io.read_model(os.path.join(REPO, "tests", "golden", "2.model"))
    assert m["no_rss"]
    drv = cd.CondDriver(m["pattern"], m["ene_param"], m["max_span"], m["max_iloop"], m["min_bpp"], m["tau"], m["flags"])
    o, x = cc.ctx_oracle_from_model(os.path.join(REPO, "tests", "golden", "2.model"))
    (s,), (q,) = synth.synth_batch(1, 40, seed=3)
    t = o.train_seq(s, q)
    kept = np.zeros((41, min(40, m["max_span"]) + 1), dtype=bool)
    for form in (0, 1):
        rec, _ = drv.record(m["x"], s, q, kept, form)
        assert len(rec["i"]) == 0 and np.all(rec["unpaired_motif"] == 1.0) and np.all(rec["unpaired_none"] == 1.0)
        assert rec["shift"] == 0.0
        assert rec["exist_prob"] == pytest.approx(np.exp(t["Zari"] - t["Zo"]), rel=1e-10)


def fake_record(rng, L, n):
    ii = np.sort(rng.integers(0, max(L - 5, 1), size=n)).astype(np.int32)
    return dict(i=ii, j=ii + 5, p_motif=rng.random(n), p_none=rng.random(n), unpaired_motif=rng.random(L), unpaired_none=rng.random(L),
                exist_prob=float(rng.random()), shift=float(rng.random() * 3), structure_motif="." * L, structure_none="(" + "." * (L - 2) + ")")


def test_record_round_trip(tmp_path):
    rng = np.random.default_rng(2)
    recs = [fake_record(rng, 9, 0), fake_record(rng, 30, 7), fake_record(rng, 12, 2)]
    recs[1]["shift"] = float("nan")
    recs[1]["p_none"][3] = 0.0
    path = tmp_path / "contrast.txt"
    path.write_text("".join(io.contrast_record("@s%d extra words" % k, r) for k, r in enumerate(recs)))
    back = io.read_contrast_records(str(path))
    assert [b["id"] for b in back] == ["@s%d extra words" % k for k in range(3)]
    for b, r in zip(back, recs):
        assert (b["structure_motif"], b["structure_none"]) == (r["structure_motif"], r["structure_none"])
        np.testing.assert_allclose(b["exist_prob"], r["exist_prob"], rtol=5e-6)
        np.testing.assert_allclose(b["shift"], r["shift"], rtol=5e-6, equal_nan=True)
        np.testing.assert_allclose(b["unpaired_motif"], r["unpaired_motif"], rtol=5e-6)
        np.testing.assert_allclose(b["unpaired_none"], r["unpaired_none"], rtol=5e-6)
        assert [(i, j) for i, j, _, _ in b["pairs"]] == [(int(i) + 1, int(j)) for i, j in zip(r["i"], r["j"])]
        np.testing.assert_allclose([p for _, _, p, _ in b["pairs"]], r["p_motif"], rtol=5e-6)
        np.testing.assert_allclose([p for _, _, _, p in b["pairs"]], r["p_none"], rtol=5e-6)
    lines = io.contrast_record("@a", recs[2]).split("\n")
    assert lines[0] == "id: @a\texist prob: %.6g\tshift: %.6g" % (recs[2]["exist_prob"], recs[2]["shift"])
    assert [l.split(": ")[0] for l in lines[1:6]] == ["motif", "none", "unpaired motif", "unpaired none", "pairs"]
    assert lines[6] == "%d %d %.6g %.6g" % (recs[2]["i"][0] + 1, recs[2]["j"][0], recs[2]["p_motif"][0], recs[2]["p_none"][0])


def test_parser_options():
    a = cli.build_parser().parse_args(["scan", "-f", "x.fq", "-q", "m.txt", "--out1", "a.raw", "--out-contrast", "c.txt"])
    assert (a.out_contrast, a.contrast_min_prob, a.contrast_gamma) == ("c.txt", 1e-3, 1.0)
    a = cli.build_parser().parse_args(["scan", "-f", "x.fq", "-q", "m.txt", "--out1", "a.raw", "--contrast-min-prob", "0.2",
                                       "--contrast-gamma", "4"])
    assert (a.out_contrast, a.contrast_min_prob, a.contrast_gamma) == (None, 0.2, 4.0)


def test_sharded_writer_joins_the_contrast_parts_of_two_ranks_in_input_order(tmp_path):
    recs = [("@r%d" % k, None, None) for k in range(5)]
    out1, outc = str(tmp_path / "scan.raw"), str(tmp_path / "contrast.txt")
    rec = fake_record(np.random.default_rng(3), 8, 2)

    def part(mine):
        for rid, _, _ in mine:
            yield "scan %s\n" % rid, io.contrast_record(rid, rec)

    for rank in (1, 0):
        cli.sharded_write(recs, [out1, outc], rank, 2, part, lambda: None)
    assert [b["id"] for b in io.read_contrast_records(outc)] == ["@r%d" % k for k in range(5)]
    assert sorted(p.name for p in tmp_path.iterdir()) == ["contrast.txt", "scan.raw"]


def test_conditional_symbols_are_declared_and_exported():
    declared = set(re.findall(r"\b(elemdp_[a-z_0-9]+)\s*\(", open(HEADER).read()))
    lib = api.load_library()
    for sym in ("elemdp_pair_conditional", "elemdp_pair_conditional_list"):
        assert sym in declared and sym in api.SYMBOLS and hasattr(lib, sym), sym
    assert hasattr(api.Engine, "conditional_pairs")
    assert "unaffected" in open(HEADER).read().split("int elemdp_pair_conditional(")[0].rsplit("/*", 1)[1]


@pytest.mark.skipif(have_gpu(), reason="only meaningful on a machine without a GPU")
def test_the_conditional_call_refuses_to_run_without_a_gpu():
    eng = api.Engine("((.*.))")
    lib = api.load_library()
    x = np.zeros(eng.n_param)
    m = C.c_int64()
    dp = C.POINTER(C.c_double)
    rc = lib.elemdp_pair_conditional(eng._h, x.ctypes.data_as(dp), eng.n_param, 0.0, 1.0, C.byref(m), None, None, None, None, None, None)
    assert rc == -2 and b"no CPU path" in lib.elemdp_last_error()      # ELEMDP_ENODEV
    assert lib.elemdp_pair_conditional_list(eng._h, None, None, None, None, None, 0) == -2
