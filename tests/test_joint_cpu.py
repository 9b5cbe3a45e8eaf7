"""Joint node-by-context posteriors and the motif logo table on the CPU: the two references of
tests/joint_check.py against each other (enumeration of structure x node row with the oracle, the definitions in numpy over the
oracle's tables); the product rule through the test-only CPU driver (tests/joint_emul.cpp), both forms and both unary forms,
against both; the marginal identities; the counts; the logo table, its file and the sharded join; the symbol."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from oracle import pyoracle as po
from rnaelem_amd import api, cli, io, synth
from tests import ctx_check as cc
from tests import joint_check as jc
from tests import node_check as nc
from tests.test_host_abi import have_gpu
from tests.util import REPO

HEADER = os.path.join(REPO, "include", "elemdp.h")
PAR = jc.PAR
P1 = "((.*.))"
SHAPES = [(20, L) for L in (1, 2, 4, 5, 19, 20, 21, 47)] + [(70, 107)]     # (W, L)
_shape = {}


def shape_reference(W, L):
    """(x, seq, qual, oracle, table joint, n_node) of a shape case, computed once"""
    if (W, L) not in _shape:
        eng = api.Engine(P1, PAR, W, 30, 1e-4, 0.1, 0, 0)
        x = jc.joint_params(eng)
        o = jc.joint_oracle(P1, W, 30)
        o.set_params(x)
        (s,), (q,) = synth.synth_batch(1, L, seed=300 + L)
        _shape[(W, L)] = (x, s, q, o, jc.table_joint(o, s, q, x), eng.n_node)
    return _shape[(W, L)]


@pytest.mark.parametrize("case", jc.CASES, ids=jc.case_id)
def test_references_agree_on_the_enumerated_cases(case):
    x, s, q, o, enum = jc.tiny_reference(case)
    assert enum is not None
    np.testing.assert_allclose(enum.sum(axis=(1, 2)), 1.0, rtol=0, atol=1e-12)
    jc.assert_joint(jc.table_joint(o, s, q, x), enum, what=case)


def test_the_enumerated_cases_cover_every_letter_on_the_inner_nodes():
    top = np.zeros(7)
    for case in jc.CASES:
        enum = jc.tiny_reference(case)[4]
        top = np.maximum(top, enum[:, 1:-1, :].sum(axis=(0, 1)))
    assert np.all(top >= 1e-3), dict(zip(cc.LETTERS, top))


@pytest.mark.parametrize("case", jc.CASES, ids=jc.case_id)
def test_product_rule_on_the_cpu_equals_the_enumeration(case):
    """joint_rules.h through the CPU driver: the scaled-linear form over the compact tables of the product's CPU sweeps (plain and
    table-driven unary phases) and the log-space form over the dense ones"""
    pattern, _, flags, min_bpp = case
    x, s, q, o, enum = jc.tiny_reference(case)
    M = enum.shape[1]
    drv = jc.JointDriver(pattern, PAR, 50, 30, min_bpp, 0.1, flags, n_node=M)
    for fast in (False, True):
        drv.set_fast(fast)
        for form in (jc.JointDriver.LIN, jc.JointDriver.LOG):
            got, counts, used = drv.joint(x, s, q, form)
            assert used == form, (case, form)
            jc.assert_joint(got, enum, what=(case, fast, form))
            np.testing.assert_allclose(got.sum(axis=(1, 2)), 1.0, rtol=0, atol=1e-12 if form == 0 else 1e-10)
            assert got.min() >= 0.0 and got.max() <= 1.0
            np.testing.assert_allclose(counts, jc.counts_of(got, s), rtol=0, atol=1e-12)


@pytest.mark.parametrize("W,L", SHAPES)
def test_product_rule_on_the_cpu_at_many_lengths(W, L):
    """beyond enumeration: the driver against the table definitions, the two marginal identities against the references of
    node_check and ctx_check (max_iloop 30), the counts against the profile, the oracle's scan identities"""
    x, s, q, o, ref, M = shape_reference(W, L)
    node_ref, ctx_ref = nc.table_profile(o, s, q, x), cc.table_profile(o, s, q, x)
    drv = jc.JointDriver(P1, PAR, W, 30, 1e-4, 0.1, 0, n_node=M)
    for fast in (False, True):
        drv.set_fast(fast)
        for form in (jc.JointDriver.LIN, jc.JointDriver.LOG):
            got, counts, used = drv.joint(x, s, q, form)
            assert used == form
            jc.assert_joint(got, ref, what=(W, L, fast, form))
            tol = 1e-12 if form == 0 else 1e-10
            np.testing.assert_allclose(got.sum(axis=(1, 2)), 1.0, rtol=0, atol=tol)
            nc.assert_profile(got.sum(axis=2), node_ref, what=(W, L, fast, form), cols=range(M))
            cc.assert_profile(got.sum(axis=1), ctx_ref, what=(W, L, fast, form))
            np.testing.assert_allclose(counts, jc.counts_of(got, s), rtol=0, atol=1e-12 * max(L, 1))
    nc.assert_oracle_identities(o, s, q, got.sum(axis=2), what=(W, L))
    assert_counts_equal_en(o, s, q, counts[None], what=(W, L))


def assert_counts_equal_en(o, seqs_or_seq, qual, counts, what=""):
    """sum over the owners of a single-base theta row of the counts summed over the letters = the oracle scan's EN of that row"""
    hmm = o.hmm()
    tid, sizes = hmm["theta_id"], hmm["theta_sizes"]
    sc = o.scan_seq(seqs_or_seq, qual)
    off = np.concatenate([[0], np.cumsum(sizes)])
    tot = counts.sum(axis=(0, 2))                                          # (M, 5)
    for r, size in enumerate(sizes):
        if size != 4:
            continue
        owners = [m for m in range(len(tid)) if tid[m] == r]
        np.testing.assert_allclose(tot[owners, 1:].sum(axis=0), sc["EN"][off[r]:off[r + 1]], rtol=1e-8, atol=1e-10, err_msg="row %d %s" % (r, what))


def test_a_dropped_chain_step_and_a_dropped_bulge_seed_are_seen():
    """the references see each term of G: without the chain step, and without seed_B, the table reference moves by more than 1e-3
    on one of the shape cases, the driver with the same term dropped follows it, and it no longer equals the whole reference"""
    for parts in (jc.PART_SEED_H | jc.PART_SEED_B, jc.PART_SEED_H | jc.PART_CHAIN):
        seen = False
        for W, L in SHAPES:
            x, s, q, o, ref, M = shape_reference(W, L)
            part_ref = jc.table_joint(o, s, q, x, parts=parts)
            if np.abs(part_ref - ref).max() <= 1e-3:
                continue
            seen = True
            got = jc.JointDriver(P1, PAR, W, 30, 1e-4, 0.1, 0, n_node=M).joint(x, s, q, 0, parts)[0]
            jc.assert_joint(got, part_ref, what=(parts, W, L))
            with pytest.raises(AssertionError):
                jc.assert_joint(got, ref)
            break
        assert seen, parts


def test_a_sequence_without_any_parse_sits_on_node_0_and_letter_O():
    o = jc.joint_oracle(P1)
    eng = api.Engine(P1, PAR, 50, 30, 1e-4, 0.1, 0, 0)
    M = eng.n_node
    x, seqs, quals = cc.no_parse_inputs(jc.joint_params(eng), o.hmm())
    o.set_params(x)
    assert jc.table_joint(o, seqs[0], quals[0], x) is None
    ref = jc.table_joint(o, seqs[1], quals[1], x)
    drv = jc.JointDriver(P1, PAR, n_node=M)
    for form in (jc.JointDriver.LIN, jc.JointDriver.LOG):
        got, counts, used = drv.joint(x, seqs[0], quals[0], form)
        assert used == jc.JointDriver.LOG and np.array_equal(got, jc.no_parse_joint(len(seqs[0]), M))
        assert np.array_equal(counts, jc.counts_of(got, seqs[0])) and counts[0, 0, 1] == len(seqs[0])
        jc.assert_joint(drv.joint(x, seqs[1], quals[1], form)[0], ref, what=form)


def test_a_model_without_structure_keeps_everything_on_rule_8():
    path = os.path.join(REPO, "tests", "golden", "2.model")
    m = io.read_model(path)
    assert m["no_rss"]
    o, x = jc.joint_oracle_from_model(path)
    M = len(o.hmm()["node"])
    drv = jc.JointDriver(m["pattern"], m["ene_param"], m["max_span"], m["max_iloop"], m["min_bpp"], m["tau"], m["flags"], n_node=M)
    for L in (3, 9, 40):       # (3: shorter than the motif, Z(ari) = 0)
        (s,), (q,) = synth.synth_batch(1, L, seed=3)
        node_ref = nc.table_profile(o, s, q, x, tau=m["tau"])
        for form in (0, 1):
            got, counts, _ = drv.joint(m["x"], s, q, form)
            assert np.all(got[:, :, 1:] == 0.0)
            nc.assert_profile(got[:, :, 0], node_ref, what=(L, form), cols=range(M))
            jc.assert_joint(got, jc.table_joint(o, s, q, x, tau=m["tau"]), what=(L, form))


def test_motif_logo():
    rng = np.random.default_rng(5)
    counts = rng.random((4, 3, 7, 5))
    counts[:, 2] = 0.0                                                       # (a node that emits nothing)
    logo = api.motif_logo(counts)
    tot = counts[0] + counts[1] + counts[2] + counts[3]
    np.testing.assert_allclose(logo["counts"], tot, rtol=1e-15)
    np.testing.assert_allclose(logo["occurrences"], tot.sum(axis=(1, 2)), rtol=1e-14)
    f = tot[:2, :, 1:].sum(axis=1)
    f /= f.sum(axis=1, keepdims=True)
    np.testing.assert_allclose(logo["base_freq"][:2], f, rtol=1e-14)
    np.testing.assert_allclose(logo["letter_freq"][:2], tot[:2].sum(axis=2) / tot[:2].sum(axis=(1, 2))[:, None], rtol=1e-14)
    np.testing.assert_allclose(logo["information"][:2], 2.0 + (f * np.log2(f)).sum(axis=1), rtol=1e-12)
    assert np.all(logo["base_freq"][2] == 0) and np.all(logo["letter_freq"][2] == 0) and logo["information"][2] == 0
    one = np.zeros((1, 1, 7, 5))
    one[0, 0, 3, 2] = 2.5                                                    # (one base only: 2 bits)
    assert api.motif_logo(one)["information"][0] == 2.0
    w = np.array([1.0, 0.0, 0.5, 0.0])
    np.testing.assert_allclose(api.motif_logo(counts, w)["counts"], counts[0] + 0.5 * counts[2], rtol=1e-15)
    with pytest.raises(ValueError):
        api.motif_logo(counts[0])
    with pytest.raises(ValueError):
        api.motif_logo(counts, [1.0])
    assert "small-sample" in api.motif_logo.__doc__


def test_logo_file_round_trip(tmp_path):
    rng = np.random.default_rng(2)
    names = "z((.*.))o"
    counts = rng.random((len(names), 7, 5)) * 10
    counts[4] = 0.0
    path = str(tmp_path / "logo.txt")
    io.write_logo(path, names, counts, 3, 5)
    back = io.read_logo(path)
    assert (back["n_used"], back["n_total"], back["names"]) == (3, 5, names)
    assert np.array_equal(back["counts"], counts)
    np.testing.assert_allclose(back["occurrences"], counts.sum(axis=(1, 2)), rtol=1e-15)
    lines = open(path).read().split("\n")
    assert lines[0] == "sequences: 3 / 5" and lines[1] == "columns: N A C G U" and lines[2] == "node: 0z"
    assert [l.split(": ")[0] for l in lines[4:11]] == list("OLRHBIM")
    recs = [("@a b", 0.25, counts), ("@c", 1.0, counts * 2)]
    parts = tmp_path / "parts.txt"
    parts.write_text("".join(io.logo_counts_record(*r) for r in recs))
    for (rid, ex, c), (rid2, ex2, c2) in zip(io.read_logo_counts(str(parts)), recs):
        assert rid == rid2 and ex == ex2 and np.array_equal(c, c2)


def test_parser_options():
    a = cli.build_parser().parse_args(["scan", "-f", "x.fq", "-q", "m.txt", "--out1", "a.raw", "--out-logo", "l.txt", "--logo-min-exist", "0.5"])
    assert (a.out_logo, a.logo_min_exist) == ("l.txt", 0.5)
    a = cli.build_parser().parse_args(["scan", "-f", "x.fq", "-q", "m.txt", "--out1", "a.raw"])
    assert a.out_logo is None and a.logo_min_exist == 0.0


def test_sharded_writer_joins_the_counts_of_two_ranks_in_input_order_before_the_sum(tmp_path):
    recs = [("@r%d" % k, None, None) for k in range(5)]
    out1, outl = str(tmp_path / "scan.raw"), str(tmp_path / "logo.txt")
    rng = np.random.default_rng(9)
    counts = {rid: rng.random((3, 7, 5)) for rid, _, _ in recs}
    exist = {rid: 0.2 * k for k, (rid, _, _) in enumerate(recs)}

    def part(mine):
        for rid, _, _ in mine:
            yield "scan %s\n" % rid, io.logo_counts_record(rid, exist[rid], counts[rid])

    for rank in (1, 0):
        cli.sharded_write(recs, [out1, outl + ".seqs"], rank, 2, part, lambda: None)
    assert [rid for rid, _, _ in io.read_logo_counts(outl + ".seqs")] == ["@r%d" % k for k in range(5)]
    cli.write_logo_from_parts(outl + ".seqs", outl, "z.o", 0.4)
    back = io.read_logo(outl)
    assert (back["n_used"], back["n_total"]) == (3, 5)
    want = np.zeros((3, 7, 5))
    for k in (2, 3, 4):                                                      # (input order)
        want += counts["@r%d" % k]
    assert np.array_equal(back["counts"], want)
    assert sorted(p.name for p in tmp_path.iterdir()) == ["logo.txt", "scan.raw"]


def test_joint_symbol_is_declared_and_exported():
    declared = set(re.findall(r"\b(elemdp_[a-z_0-9]+)\s*\(", open(HEADER).read()))
    assert "elemdp_joint_profile" in declared and "elemdp_joint_profile" in api.SYMBOLS
    assert hasattr(api.load_library(), "elemdp_joint_profile")
    assert hasattr(api.Engine, "joint_profiles") and callable(api.motif_logo)


@pytest.mark.skipif(have_gpu(), reason="only meaningful on a machine without a GPU")
def test_a_call_without_a_device_is_refused():
    eng = api.Engine(P1, PAR, 50, 30, 1e-4, 0.1, 0, 0)
    x = np.zeros(eng.n_param)
    out = np.zeros(35 * eng.n_node)
    dp = C.POINTER(C.c_double)
    assert api.load_library().elemdp_joint_profile(eng._h, x.ctypes.data_as(dp), eng.n_param, out.ctypes.data_as(dp), None) == -2     # ELEMDP_ENODEV
