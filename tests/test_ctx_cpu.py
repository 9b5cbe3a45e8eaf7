"""Structural context profiles on the CPU: the definitions of ctx_rules.h over the oracle's tables
(ctx_check.table_profile) against brute-force enumeration with the oracle (ctx_check.enumerated_profile); the product rule
through the test-only CPU driver (tests/ctx_emul.cpp), both forms, against both references; the letters of sampled structures
against the classifier the enumeration uses; the record format, the parser, the sharded writer and the symbol."""
import os
import re

import numpy as np
import pytest

from oracle import pyoracle as po
from rnaelem_amd import api, cli, io, synth
from tests import ctx_check as cc
from tests.sample_check import Driver, dot_bracket
from tests.test_pair_posterior_gpu import PAR, perturbed
from tests.util import REPO

HEADER = os.path.join(REPO, "include", "elemdp.h")
PATTERNS = ["((.*.))", "(.*)", "(.....)"]
LENGTHS = (12, 15, 18, 20)         # (synth seed 100 + L; the 15-mer under `(.*)` without energies reaches M = 0.014, the 20-mer 0.04)
CASES = [(p, f, b) for p in PATTERNS for f in (0, po.NO_ENE) for b in (0.0, 1e-4)]
_refs = {}


def case_inputs(case):
    pattern, flags, min_bpp = case
    x = perturbed(api.Engine(pattern, PAR, 50, 30, min_bpp, 0.1, flags, 0))
    seqs, quals = [], []
    for L in LENGTHS:
        (s,), (q,) = synth.synth_batch(1, L, seed=100 + L)
        seqs.append(s)
        quals.append(q)
    return x, seqs, quals


def references(case):
    """(x, seqs, quals, enumerated profiles, table profiles) of a case, computed once"""
    if case not in _refs:
        pattern, flags, min_bpp = case
        x, seqs, quals = case_inputs(case)
        o = cc.ctx_oracle(pattern, 50, 30, min_bpp=min_bpp, flags=flags)
        o.set_params(x)
        enum = [cc.enumerated_profile(o, s, q) for s, q in zip(seqs, quals)]
        tab = [cc.table_profile(o, s, q, x) for s, q in zip(seqs, quals)]
        _refs[case] = (x, seqs, quals, enum, tab)
    return _refs[case]


def test_classifier_letters():
    assert cc.classify("..((...))..") == "OOLLHHHRROO"
    assert cc.classify("(.((...)))") == "LBLLHHHRRR"
    assert cc.classify("(((...)).)") == "LLLHHHRRBR"
    assert cc.classify("(.((...)).)") == "LILLHHHRRIR"
    assert cc.classify("((...).(...))") == "LLHHHRMLHHHRR"
    assert cc.classify("(...)(...)") == "LHHHRLHHHR"


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%s-%d-%g" % c)
def test_table_definitions_equal_the_enumeration(case):
    x, seqs, quals, enum, tab = references(case)
    assert sum(e is not None for e in enum) >= 3
    for k, (e, t) in enumerate(zip(enum, tab)):
        assert (e is None) == (t is None), k
        if e is None:
            continue
        cc.assert_profile(t, e, what=(case, k))
        np.testing.assert_allclose(e.sum(axis=1), 1.0, rtol=0, atol=1e-12)


def test_every_column_is_covered_by_the_cases():
    top = np.zeros(7)
    for case in CASES:
        for e in references(case)[3]:
            if e is not None:
                top = np.maximum(top, e.max(axis=0))
    assert np.all(top > 1e-3), dict(zip(cc.LETTERS, top))


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%s-%d-%g" % c)
def test_product_rule_on_the_cpu_equals_both_references(case):
    """ctx_rules.h through the CPU driver: the scaled-linear form over the compact tables of the product's CPU sweeps (plain and
    table-driven unary phases) and the log-space form over the dense ones"""
    pattern, flags, min_bpp = case
    x, seqs, quals, enum, tab = references(case)
    drv = cc.CtxDriver(pattern, PAR, 50, 30, min_bpp, 0.1, flags)
    for fast in (False, True):
        drv.set_fast(fast)
        for k, (s, q) in enumerate(zip(seqs, quals)):
            for form in (cc.CtxDriver.LIN, cc.CtxDriver.LOG):
                got, used = drv.profile(x, s, q, form)
                if enum[k] is None:
                    assert used == cc.CtxDriver.LOG and np.array_equal(got, cc.exterior_only(len(s))), (case, k)
                    continue
                assert used == form, (case, k, form)
                cc.assert_profile(got, enum[k], what=(case, k, form, "enumerated"))
                cc.assert_profile(got, tab[k], what=(case, k, form, "tables"))
                np.testing.assert_allclose(got.sum(axis=1), 1.0, rtol=0, atol=1e-12)
                assert got.min() >= 0.0 and got.max() <= 1.0


def test_sequences_without_a_parse_and_models_without_structure_are_all_exterior():
    drv = cc.CtxDriver("(.........)", PAR, 50, 30, 1e-4, 0.1, 0)
    x = perturbed(api.Engine("(.........)", PAR, 50, 30, 1e-4, 0.1, 0, 0))
    s = np.zeros(30, dtype=np.uint8)
    q = np.full(31, 10, dtype=np.uint8)
    q[-1] = 0
    o = cc.ctx_oracle("(.........)")
    o.set_params(x)
    for form in (0, 1):
        got, _ = drv.profile(x, s, q, form)
        ref = cc.table_profile(o, s, q, x)
        if ref is None:
            assert np.array_equal(got, cc.exterior_only(30))
        else:          # (all N keeps no pair: the one structure is the open chain)
            cc.assert_profile(got, ref)
            assert np.all(got[:, 0] > 1.0 - 1e-12)
    m = io.read_model(os.path.join(REPO, "tests", "golden", "2.model"))
    assert m["no_rss"]
    drv = cc.CtxDriver(m["pattern"], m["ene_param"], m["max_span"], m["max_iloop"], m["min_bpp"], m["tau"], m["flags"])
    (s,), (q,) = synth.synth_batch(1, 40, seed=3)
    for form in (0, 1):
        assert np.array_equal(drv.profile(m["x"], s, q, form)[0], cc.exterior_only(40))


def test_a_sequence_without_any_parse_is_exactly_exterior():
    """theta(A) = -inf: poly-A has Z(ari, nasi) = 0, the scaled-linear form hands it on and the log-space form writes O = 1 and
    zeros exactly; the sequence without A next to it keeps its profile"""
    pattern = "((.*.))"
    o = cc.ctx_oracle(pattern)
    x, seqs, quals = cc.no_parse_inputs(perturbed(api.Engine(pattern, PAR, 50, 30, 1e-4, 0.1, 0, 0)), o.hmm())
    o.set_params(x)
    assert o.derivation_logz(seqs[0], quals[0], None, None) == -np.inf and cc.table_profile(o, seqs[0], quals[0], x) is None
    ref = cc.table_profile(o, seqs[1], quals[1], x)
    assert ref is not None and ref[:, 1].max() > 0.1
    drv = cc.CtxDriver(pattern, PAR)
    for form in (cc.CtxDriver.LIN, cc.CtxDriver.LOG):
        got, used = drv.profile(x, seqs[0], quals[0], form)
        assert used == cc.CtxDriver.LOG and np.array_equal(got, cc.exterior_only(len(seqs[0])))
        cc.assert_profile(drv.profile(x, seqs[1], quals[1], form)[0], ref, what=form)


@pytest.mark.parametrize("pattern", ["((.*.))", "(.....)"])
def test_sampled_letters_follow_the_classifier(pattern):
    """the rss letters scan and the sampler print are the classifier's letters of their own dot-bracket: the B / I / M convention
    of the profile is the one of the single parses"""
    x = perturbed(api.Engine(pattern, PAR, 50, 30, 1e-4, 0.1, 0, 0))
    drv = Driver(pattern, PAR)
    seen = set()
    for L in (20, 40, 97):
        (s,), (q,) = synth.synth_batch(1, L, seed=900 + L)
        rss, _, _, st = drv.sample(x, s, q, 300, 5, 0)
        assert st == 0
        for r in set(rss):
            assert cc.classify(dot_bracket(r)) == r, (pattern, L, r)
            seen |= set(r)
    assert set("OLRHBI") <= seen, seen


def test_record_round_trip(tmp_path):
    rng = np.random.default_rng(1)
    profs = [rng.dirichlet(np.ones(7), size=L) for L in (1, 9, 30)]
    profs[1][3, 2] = 0.0
    path = tmp_path / "ctx.txt"
    path.write_text("".join(io.context_record("@s%d extra words" % k, p) for k, p in enumerate(profs)))
    back = io.read_context_records(str(path))
    assert [rid for rid, _ in back] == ["@s%d extra words" % k for k in range(3)]
    for (_, b), p in zip(back, profs):
        assert b.shape == p.shape
        np.testing.assert_allclose(b, p, rtol=5e-6, atol=0)
    text = io.context_record("@a", profs[0])
    assert text.split("\n")[0] == "id: @a" and [l[:3] for l in text.split("\n")[1:8]] == ["%s: " % c for c in "OLRHBIM"]
    assert text.split("\n")[1] == "O: [%.6g]" % profs[0][0, 0]


def test_parser_options():
    a = cli.build_parser().parse_args(["scan", "-f", "x.fq", "-q", "m.txt", "--out1", "a.raw", "--out-context", "c.txt",
                                       "--out-pairs", "p.txt", "--out-mea", "m.txt", "--out-samples", "s.txt"])
    assert (a.out_context, a.out_pairs, a.out_mea, a.out_samples) == ("c.txt", "p.txt", "m.txt", "s.txt")
    a = cli.build_parser().parse_args(["scan", "-f", "x.fq", "-q", "m.txt", "--out1", "a.raw"])
    assert a.out_context is None


def test_sharded_writer_joins_the_context_parts_of_two_ranks_in_input_order(tmp_path):
    recs = [("@r%d" % k, None, None) for k in range(5)]
    out1, outc = str(tmp_path / "scan.raw"), str(tmp_path / "ctx.txt")
    prof = np.full((2, 7), 1.0 / 7)

    def part(mine):
        for rid, _, _ in mine:
            yield "scan %s\n" % rid, io.context_record(rid, prof)

    for rank in (1, 0):
        cli.sharded_write(recs, [out1, outc], rank, 2, part, lambda: None)
    assert open(out1).read() == "".join("scan @r%d\n" % k for k in range(5))
    assert [rid for rid, _ in io.read_context_records(outc)] == ["@r%d" % k for k in range(5)]
    assert sorted(p.name for p in tmp_path.iterdir()) == ["ctx.txt", "scan.raw"]


def test_context_symbol_is_declared_and_exported():
    declared = set(re.findall(r"\b(elemdp_[a-z_0-9]+)\s*\(", open(HEADER).read()))
    assert "elemdp_context_profile" in declared and "elemdp_context_profile" in api.SYMBOLS
    assert hasattr(api.load_library(), "elemdp_context_profile")
    assert hasattr(api.Engine, "context_profiles")
