"""Posterior motif-node profiles on the CPU: the three references of tests/node_check.py against each other
(enumeration with the oracle, the oracle's scan identities, the definitions in numpy over the oracle's tables); the product rule
through the test-only CPU driver (tests/node_emul.cpp), both forms and both unary forms, against all three; the record format,
the parser, the confidence of an alignment and the symbol."""
import os
import re

import numpy as np
import pytest

from oracle import pyoracle as po
from rnaelem_amd import api, cli, io, synth
from tests import ctx_check as cc
from tests import node_check as nc
from tests.test_pair_posterior_gpu import PAR
from tests.util import REPO

HEADER = os.path.join(REPO, "include", "elemdp.h")
TINY = [("(.....)", 13), ("((...))", 14), ("((.*.))", 14)]       # (pattern, L): the sizes the enumeration affords
CASES = [(p, L, f, b) for p, L in TINY for f in (0, po.NO_ENE) for b in (0.0, 1e-4)]
P1, P2 = "((.*.))", "(.....)"                                   # the patterns of test_pair_shapes_gpu
SHAPE_LENS = (1, 2, 5, 49, 50, 51, 107)
_refs = {}


def node_params(eng):
    """perturbed initial parameters with lambda = (1.0, 0.7)"""
    x = eng.initial_params(1.0)
    x[:-2] += np.linspace(-0.3, 0.3, len(x) - 2)
    x[-2:] = (1.0, 0.7)
    return x


def tiny_inputs(case):
    pattern, L, flags, min_bpp = case
    x = node_params(api.Engine(pattern, PAR, 50, 30, min_bpp, 0.1, flags, 0))
    (s,), (q,) = synth.synth_batch(1, L, seed=100 + L)
    return x, s, q


def tiny_reference(case):
    """(x, seq, qual, oracle, enumerated profile) of a tiny case, computed once"""
    if case not in _refs:
        pattern, L, flags, min_bpp = case
        x, s, q = tiny_inputs(case)
        o = nc.node_oracle(pattern, 50, 30, min_bpp=min_bpp, flags=flags)
        o.set_params(x)
        _refs[case] = (x, s, q, o, nc.enumerated_profile(o, s, q))
    return _refs[case]


def test_alignment_rows():
    rows = ["".join("z(.)o"[h] for h in r) for r in nc.alignments(4, "z(.)o")]
    assert rows[0] == "zzzz" and len(set(rows)) == len(rows)
    assert set(rows) == {"zzzz", "(.)o", "z(.)", "((.)", "(..)", "(.))"}
    star = ["".join("z.*o"[h] for h in r) for r in nc.alignments(2, "z.*o")]
    assert set(star) == {"zz", ".o", "z.", "..", ".*"}


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%s-%d-%d-%g" % c)
def test_references_agree_on_the_tiny_batch(case):
    x, s, q, o, enum = tiny_reference(case)
    assert enum is not None
    np.testing.assert_allclose(enum.sum(axis=1), 1.0, rtol=0, atol=1e-12)
    nc.assert_oracle_identities(o, s, q, enum, what=case)
    nc.assert_profile(nc.table_profile(o, s, q, x), enum, what=case, cols=range(enum.shape[1]))


def test_the_tiny_batch_is_not_vacuous():
    for pattern, L in TINY:
        top, inner = None, 0.0
        for case in CASES:
            if case[0] != pattern:
                continue
            enum = tiny_reference(case)[4]
            top = enum.max(axis=0) if top is None else np.maximum(top, enum.max(axis=0))
            inner = max(inner, enum[:, 1:-1].sum(axis=1).max())
        assert inner >= 0.05, (pattern, inner)
        assert np.all(top >= 1e-3), (pattern, top)


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%s-%d-%d-%g" % c)
def test_product_rule_on_the_cpu_equals_the_enumeration(case):
    """node_rules.h through the CPU driver: the scaled-linear form over the compact tables of the product's CPU sweeps (plain and
    table-driven unary phases) and the log-space form over the dense ones"""
    pattern, L, flags, min_bpp = case
    x, s, q, o, enum = tiny_reference(case)
    M = enum.shape[1]
    drv = nc.NodeDriver(pattern, PAR, 50, 30, min_bpp, 0.1, flags, n_node=M)
    for fast in (False, True):
        drv.set_fast(fast)
        for form in (nc.NodeDriver.LIN, nc.NodeDriver.LOG):
            got, used = drv.profile(x, s, q, form)
            assert used == form, (case, form)
            nc.assert_profile(got, enum, what=(case, fast, form), cols=range(M))
            np.testing.assert_allclose(got.sum(axis=1), 1.0, rtol=0, atol=1e-12)
            assert got.min() >= 0.0 and got.max() <= 1.0


@pytest.mark.parametrize("pattern,W", [(P1, 50), (P2, 50), (P1, 20)])
def test_product_rule_on_the_cpu_at_many_lengths(pattern, W):
    """beyond enumeration: the driver against the table definitions (per position and node) and the oracle's scan identities"""
    eng = api.Engine(pattern, PAR, W, 30, 1e-4, 0.1, 0, 0)
    x = node_params(eng)
    M = eng.n_node
    o = nc.node_oracle(pattern, W, 30)
    o.set_params(x)
    drv = nc.NodeDriver(pattern, PAR, W, 30, 1e-4, 0.1, 0, n_node=M)
    for L in SHAPE_LENS:
        (s,), (q,) = synth.synth_batch(1, L, seed=300 + L)
        ref = nc.table_profile(o, s, q, x)
        for fast in (False, True):
            drv.set_fast(fast)
            for form in (nc.NodeDriver.LIN, nc.NodeDriver.LOG):
                got, used = drv.profile(x, s, q, form)
                assert used == form
                nc.assert_profile(got, ref, what=(pattern, W, L, fast, form), cols=range(M))
                np.testing.assert_allclose(got.sum(axis=1), 1.0, rtol=0, atol=1e-12)
        nc.assert_oracle_identities(o, s, q, got, what=(pattern, W, L))


def test_a_sequence_without_any_parse_sits_on_node_0():
    pattern = P1
    o = nc.node_oracle(pattern)
    eng = api.Engine(pattern, PAR, 50, 30, 1e-4, 0.1, 0, 0)
    x, seqs, quals = cc.no_parse_inputs(node_params(eng), o.hmm())
    o.set_params(x)
    assert nc.table_profile(o, seqs[0], quals[0], x) is None
    ref = nc.table_profile(o, seqs[1], quals[1], x)
    drv = nc.NodeDriver(pattern, PAR, n_node=eng.n_node)
    for form in (nc.NodeDriver.LIN, nc.NodeDriver.LOG):
        got, used = drv.profile(x, seqs[0], quals[0], form)
        assert used == nc.NodeDriver.LOG and np.array_equal(got, nc.no_parse_profile(len(seqs[0]), eng.n_node))
        nc.assert_profile(drv.profile(x, seqs[1], quals[1], form)[0], ref, what=form, cols=range(eng.n_node))


def test_a_model_without_structure_keeps_the_alignment_on_rule_8():
    path = os.path.join(REPO, "tests", "golden", "2.model")
    m = io.read_model(path)
    assert m["no_rss"]
    o, x = nc.node_oracle_from_model(path)
    M = len(o.hmm()["node"])
    drv = nc.NodeDriver(m["pattern"], m["ene_param"], m["max_span"], m["max_iloop"], m["min_bpp"], m["tau"], m["flags"], n_node=M)
    for L in (3, 9, 40):       # (3: shorter than the motif, Z(ari) = 0)
        (s,), (q,) = synth.synth_batch(1, L, seed=3)
        for form in (0, 1):
            got, _ = drv.profile(m["x"], s, q, form)
            np.testing.assert_allclose(got.sum(axis=1), 1.0, rtol=0, atol=1e-12)
            nc.assert_oracle_identities(o, s, q, got, what=(L, form))
            nc.assert_profile(got, nc.table_profile(o, s, q, x, tau=m["tau"]), what=(L, form), cols=range(M))


def test_record_round_trip(tmp_path):
    rng = np.random.default_rng(1)
    names = "z((.*.))o"
    profs = [rng.dirichlet(np.ones(len(names)), size=L) for L in (1, 9, 30)]
    profs[1][3, 2] = 0.0
    p1 = profs[1].max(axis=1)
    confs = [None, p1, None]
    path = tmp_path / "nodes.txt"
    path.write_text("".join(io.node_record("@s%d extra words" % k, p, names, c) for k, (p, c) in enumerate(zip(profs, confs))))
    back = io.read_node_records(str(path))
    assert [rid for rid, _, _, _ in back] == ["@s%d extra words" % k for k in range(3)]
    for (_, nm, b, c), p, conf in zip(back, profs, confs):
        assert nm == names and b.shape == p.shape and (c is None) == (conf is None)
        np.testing.assert_allclose(b, p, rtol=5e-6, atol=0)
    np.testing.assert_allclose(back[1][3], p1, rtol=5e-6, atol=0)
    text = io.node_record("@a", profs[0], names)
    lines = text.split("\n")
    assert lines[0] == "id: @a" and [l.split(": ")[0] for l in lines[1:10]] == ["%d%s" % (k, c) for k, c in enumerate(names)]
    assert lines[1] == "0z: [%.6g]" % profs[0][0, 0] and lines[10] == ""


def test_alignment_confidence():
    prof = np.array([[0.9, 0.1, 0.0], [0.2, 0.5, 0.3], [0.0, 0.25, 0.75]])
    assert np.array_equal(api.alignment_confidence(prof, [0, 1, 2]), [0.9, 0.5, 0.75])
    assert np.array_equal(api.alignment_confidence(prof, np.array([1, 0, 0], dtype=np.int32)), [0.1, 0.2, 0.0])
    assert api.alignment_confidence(np.zeros((0, 3)), []).shape == (0,)
    with pytest.raises(ValueError):
        api.alignment_confidence(prof, [0, 1])
    with pytest.raises(ValueError):
        api.alignment_confidence(prof, [0, 1, 3])


def test_parser_option():
    a = cli.build_parser().parse_args(["scan", "-f", "x.fq", "-q", "m.txt", "--out1", "a.raw", "--out-nodes", "n.txt", "--out-context", "c.txt"])
    assert (a.out_nodes, a.out_context) == ("n.txt", "c.txt")
    assert cli.build_parser().parse_args(["scan", "-f", "x.fq", "-q", "m.txt", "--out1", "a.raw"]).out_nodes is None


def test_sharded_writer_joins_the_node_parts_of_two_ranks_in_input_order(tmp_path):
    recs = [("@r%d" % k, None, None) for k in range(5)]
    out1, outn = str(tmp_path / "scan.raw"), str(tmp_path / "nodes.txt")
    prof = np.full((2, 3), 1.0 / 3)

    def part(mine):
        for rid, _, _ in mine:
            yield "scan %s\n" % rid, io.node_record(rid, prof, "z.o")

    for rank in (1, 0):
        cli.sharded_write(recs, [out1, outn], rank, 2, part, lambda: None)
    assert [rid for rid, _, _, _ in io.read_node_records(outn)] == ["@r%d" % k for k in range(5)]


def test_node_symbol_is_declared_and_exported():
    declared = set(re.findall(r"\b(elemdp_[a-z_0-9]+)\s*\(", open(HEADER).read()))
    assert "elemdp_node_profile" in declared and "elemdp_node_profile" in api.SYMBOLS
    assert hasattr(api.load_library(), "elemdp_node_profile")
    assert hasattr(api.Engine, "node_profiles") and callable(api.alignment_confidence)
