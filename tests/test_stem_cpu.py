"""Pair posteriors by motif node pair and the stem logo table on the CPU: the references of
tests/stem_check.py against each other (enumeration of structure x node row with the oracle, the definition in numpy over the
oracle's tables, the oracle's own scan); the product rule through the test-only CPU driver (tests/stem_emul.cpp), both forms and
both unary forms, against them; the identities with the pair, node and joint references; the counts; the logo table, its file
and the sharded join; the symbols."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from oracle import pyoracle as po
from rnaelem_amd import api, cli, io, synth
from tests import ctx_check as cc
from tests import joint_check as jc
from tests import pair_check as pc
from tests import stem_check as sc
from tests.test_host_abi import have_gpu
from tests.util import REPO

HEADER = os.path.join(REPO, "include", "elemdp.h")
PAR = sc.PAR
P1 = "((.*.))"
SHAPES = [(20, L) for L in (1, 2, 4, 5, 19, 20, 21, 47)] + [(70, 107)]     # (W, L)
_shape = {}

# every test of this file belongs to the stem call: without its symbols the module does not import
assert all(name in api.SYMBOLS for name in ("elemdp_stem_slots", "elemdp_stem_profile", "elemdp_stem_list"))


def shape_reference(W, L):
    """(x, seq, qual, oracle, table Q) of a shape case, computed once"""
    if (W, L) not in _shape:
        eng = api.Engine(P1, PAR, W, 30, 1e-4, 0.1, 0, 0)
        x = sc.stem_params(eng)
        o = sc.stem_oracle(P1, W, 30)
        o.set_params(x)
        (s,), (q,) = synth.synth_batch(1, L, seed=300 + L)
        _shape[(W, L)] = (x, s, q, o, sc.table_stems(o, s, q, x))
    return _shape[(W, L)]


@pytest.mark.parametrize("case", sc.CASES, ids=sc.case_id)
def test_references_agree_on_the_enumerated_cases(case):
    x, s, q, o, enum = sc.tiny_reference(case)
    assert enum is not None
    sc.assert_stem(sc.table_stems(o, s, q, x), enum, what=case)


def test_the_enumerated_cases_cover_the_pattern_pairs_the_enclosing_pair_and_the_background_pairs():
    """conditions on the reference, with wide room over the values seen: every pattern pair and the z-o pair in every case;
    the *-* and o-o pairs where the sequence is long enough for a pair inside '*' and one behind the motif"""
    for case in sc.CASES:
        enum = sc.tiny_reference(case)[4]
        names = sc.tiny_reference(case)[3].hmm()["node"]
        mass = enum.sum(axis=(0, 1))
        for l, r in sc.pattern_pairs(names):
            assert mass[l, r] >= 1e-3, (case, l, r, mass[l, r])
        assert mass[0, len(names) - 1] >= 1e-3, (case, mass[0, len(names) - 1])
    case = ("(.*)", 16, po.NO_ENE, 0.0)
    assert case in sc.CASES
    names = sc.tiny_reference(case)[3].hmm()["node"]
    mass = sc.tiny_reference(case)[4].sum(axis=(0, 1))
    star, o_ = names.index("*"), len(names) - 1
    assert mass[star, star] >= 1e-3 and mass[o_, o_] >= 1e-3, (mass[star, star], mass[o_, o_])


@pytest.mark.parametrize("case", sc.CASES, ids=sc.case_id)
def test_product_rule_on_the_cpu_equals_the_enumeration(case):
    """stem_rules.h through the CPU driver: the scaled-linear form over the compact tables of the product's CPU sweeps (plain and
    table-driven unary phases) and the log-space form over the dense ones"""
    pattern, _, flags, min_bpp = case
    x, s, q, o, enum = sc.tiny_reference(case)
    drv = sc.StemDriver(pattern, PAR, 50, 30, min_bpp, 0.1, flags)
    ref = sc.by_slot(enum, drv.slots)              # (a slot the enumeration reaches is a slot of the product)
    for fast in (False, True):
        drv.set_fast(fast)
        for form in (sc.StemDriver.LIN, sc.StemDriver.LOG):
            got, counts, used = drv.stems(x, s, q, form)
            assert used == form, (case, form)
            sc.assert_stem(got, ref, what=(case, fast, form))
            assert got.min() >= 0.0 and got.max() <= 1.0
            np.testing.assert_allclose(counts, sc.counts_of(got, s), rtol=0, atol=1e-12)
    assert sc.assert_counts_equal_en(o, s, q, counts, drv.slots, what=case) > 0


@pytest.mark.parametrize("W,L", SHAPES)
def test_product_rule_on_the_cpu_at_many_lengths(W, L):
    """beyond enumeration: the driver against the table definition; sum_k Q against the P of the pair reference; the two count
    marginals against the L and R columns of the joint reference's counts; the counts by pair type against the oracle's scan"""
    x, s, q, o, ref = shape_reference(W, L)
    drv = sc.StemDriver(P1, PAR, W, 30, 1e-4, 0.1, 0)
    ref = sc.by_slot(ref, drv.slots)
    P = pc.oracle_pairs(o, s, q)
    jcounts = jc.counts_of(jc.table_joint(o, s, q, x), s)                   # (M, 7, 5)
    for fast in (False, True):
        drv.set_fast(fast)
        for form in (sc.StemDriver.LIN, sc.StemDriver.LOG):
            got, counts, used = drv.stems(x, s, q, form)
            assert used == form
            sc.assert_stem(got, ref, what=(W, L, fast, form))
            np.testing.assert_allclose(counts, sc.counts_of(got, s), rtol=0, atol=1e-12 * max(L, 1))
            tot = got.sum(axis=2)
            for i in range(L):
                for d in range(1, min(P.shape[1] - 1, L - i) + 1):
                    assert tot[i, i + d] == pytest.approx(P[i, d], rel=1e-8, abs=1e-10), (W, L, fast, form, i, d)
            for m in range(jcounts.shape[0]):
                left = sum(counts[k].sum(axis=1) for k in range(len(drv.slots)) if drv.slots[k, 0] == m) + np.zeros(5)
                right = sum(counts[k].sum(axis=0) for k in range(len(drv.slots)) if drv.slots[k, 1] == m) + np.zeros(5)
                sc.assert_stem(left, jcounts[m, jc.L_], what=(W, L, fast, form, m, "L"))
                sc.assert_stem(right, jcounts[m, jc.R_], what=(W, L, fast, form, m, "R"))
    seen = sc.assert_counts_equal_en(o, s, q, counts, drv.slots, what=(W, L))
    assert seen == 12                                                        # (two ')' nodes, six types each)


def test_a_dropped_stacking_term_is_seen():
    """the references see the 1b term: without it the table reference moves by more than 1e-3 on a shape case with energies, the
    driver with the same term dropped follows it, and it no longer equals the whole reference"""
    seen = False
    for W, L in SHAPES:
        x, s, q, o, ref = shape_reference(W, L)
        part_ref = sc.table_stems(o, s, q, x, parts=sc.PART_1A)
        if np.abs(part_ref - ref).max() <= 1e-3:
            continue
        seen = True
        drv = sc.StemDriver(P1, PAR, W, 30, 1e-4, 0.1, 0)
        got = drv.stems(x, s, q, 0, sc.PART_1A)[0]
        sc.assert_stem(got, sc.by_slot(part_ref, drv.slots), what=(W, L))
        with pytest.raises(AssertionError):
            sc.assert_stem(got, sc.by_slot(ref, drv.slots))
        break
    assert seen


def test_a_sequence_without_any_parse_has_no_stems():
    o = sc.stem_oracle(P1)
    eng = api.Engine(P1, PAR, 50, 30, 1e-4, 0.1, 0, 0)
    x, seqs, quals = cc.no_parse_inputs(sc.stem_params(eng), o.hmm())
    o.set_params(x)
    assert sc.table_stems(o, seqs[0], quals[0], x) is None
    drv = sc.StemDriver(P1, PAR)
    ref = sc.by_slot(sc.table_stems(o, seqs[1], quals[1], x), drv.slots)
    for form in (sc.StemDriver.LIN, sc.StemDriver.LOG):
        got, counts, used = drv.stems(x, seqs[0], quals[0], form)
        assert used == sc.StemDriver.LOG and not got.any() and not counts.any()
        sc.assert_stem(drv.stems(x, seqs[1], quals[1], form)[0], ref, what=form)


def test_a_model_without_structure_has_no_stems():
    path = os.path.join(REPO, "tests", "golden", "2.model")
    m = io.read_model(path)
    assert m["no_rss"]
    o, x = sc.stem_oracle_from_model(path)
    drv = sc.StemDriver(m["pattern"], m["ene_param"], m["max_span"], m["max_iloop"], m["min_bpp"], m["tau"], m["flags"])
    for L in (3, 9, 40):
        (s,), (q,) = synth.synth_batch(1, L, seed=3)
        ref = sc.table_stems(o, s, q, x, tau=m["tau"])
        assert ref is None or not ref.any()
        for form in (0, 1):
            got, counts, _ = drv.stems(m["x"], s, q, form)
            assert not got.any() and not counts.any()


def test_stem_logo():
    rng = np.random.default_rng(5)
    slots = np.array([[0, 0], [1, 3], [2, 2]])
    names = "z(.)o"
    counts = rng.random((4, 3, 5, 5))
    counts[:, 2] = 0.0                                                       # (a slot that emits nothing)
    logo = api.stem_logo(counts, slots, names)
    tot = counts[0] + counts[1] + counts[2] + counts[3]
    np.testing.assert_allclose(logo["counts"], tot, rtol=1e-15)
    np.testing.assert_allclose(logo["occurrences"], tot.sum(axis=(1, 2)), rtol=1e-14)
    assert logo["labels"] == ["0z-0z", "1(-3)", "2.-2."]
    code = dict(N=0, A=1, C=2, G=3, U=4)
    assert api.STEM_PAIR_TYPES == ("CG", "GC", "GU", "UG", "AU", "UA")
    canon = np.stack([tot[:, code[t[0]], code[t[1]]] for t in api.STEM_PAIR_TYPES], axis=1)
    occ = tot.sum(axis=(1, 2))
    np.testing.assert_allclose(logo["pair_freq"][:2, :6], canon[:2] / occ[:2, None], rtol=1e-14)
    np.testing.assert_allclose(logo["pair_freq"][:2].sum(axis=1), 1.0, rtol=1e-14)
    f6 = canon[:2] / canon[:2].sum(axis=1, keepdims=True)
    np.testing.assert_allclose(logo["information"][:2], np.log2(6.0) + (f6 * np.log2(f6)).sum(axis=1), rtol=1e-12)
    j = tot[:2, 1:, 1:] / tot[:2, 1:, 1:].sum(axis=(1, 2), keepdims=True)
    mi = (j * np.log2(j / (j.sum(axis=2, keepdims=True) * j.sum(axis=1, keepdims=True)))).sum(axis=(1, 2))
    np.testing.assert_allclose(logo["mutual_information"][:2], mi, rtol=1e-10, atol=1e-14)
    assert not logo["pair_freq"][2].any() and logo["information"][2] == 0 and logo["mutual_information"][2] == 0
    # an outer-product block: the two columns are independent
    outer = np.zeros((1, 1, 5, 5))
    outer[0, 0, 1:, 1:] = np.outer([0.1, 0.2, 0.3, 0.4], [0.4, 0.3, 0.2, 0.1])
    assert abs(api.stem_logo(outer, [[1, 3]], names)["mutual_information"][0]) <= 1e-14
    # perfect covariation over the four Watson-Crick pairs: 2 bits; one pair type only: log2(6) bits of information
    wc = np.zeros((1, 1, 5, 5))
    for a, b in ("AU", "UA", "CG", "GC"):
        wc[0, 0, code[a], code[b]] = 2.5
    assert api.stem_logo(wc, [[1, 3]], names)["mutual_information"][0] == pytest.approx(2.0, abs=1e-14)
    one = np.zeros((1, 1, 5, 5))
    one[0, 0, code["G"], code["C"]] = 0.3
    l1 = api.stem_logo(one, [[1, 3]], names)
    assert l1["information"][0] == pytest.approx(np.log2(6.0)) and l1["pair_freq"][0].tolist() == [0, 1, 0, 0, 0, 0, 0]
    w = np.array([1.0, 0.0, 0.5, 0.0])
    np.testing.assert_allclose(api.stem_logo(counts, slots, names, w)["counts"], counts[0] + 0.5 * counts[2], rtol=1e-15)
    with pytest.raises(ValueError):
        api.stem_logo(counts[0], slots, names)
    with pytest.raises(ValueError):
        api.stem_logo(counts, slots, names, [1.0])
    with pytest.raises(ValueError):
        api.stem_logo(counts, slots[:2], names)
    assert "small-sample" in api.stem_logo.__doc__


def test_stems_file_round_trip(tmp_path):
    rng = np.random.default_rng(2)
    names = "z((.*.))o"
    slots = np.array([[0, 0], [0, 8], [1, 7], [2, 6], [4, 4], [8, 8]])
    counts = rng.random((len(slots), 5, 5)) * 10
    counts[4] = 0.0
    path = str(tmp_path / "stems.txt")
    io.write_stems(path, names, slots, counts, 3, 5)
    back = io.read_stems(path)
    assert (back["n_used"], back["n_total"]) == (3, 5)
    assert np.array_equal(back["slots"], slots) and back["names"][2] == ("(", ")")
    assert np.array_equal(back["counts"], counts)
    np.testing.assert_allclose(back["occurrences"], counts.sum(axis=(1, 2)), rtol=1e-15)
    lines = open(path).read().split("\n")
    assert lines[0] == "sequences: 3 / 5" and lines[1] == "columns: N A C G U" and lines[2] == "stem: 0z 0z" and lines[16] == "stem: 1( 7)"
    assert [l.split(": ")[0] for l in lines[4:9]] == list("NACGU")
    recs = [("@a b", 0.25, counts), ("@c", 1.0, counts * 2)]
    parts = tmp_path / "parts.txt"
    parts.write_text("".join(io.stem_counts_record(*r) for r in recs))
    for (rid, ex, c), (rid2, ex2, c2) in zip(io.read_stem_counts(str(parts)), recs):
        assert rid == rid2 and ex == ex2 and np.array_equal(c, c2)
    assert io.stem_pair_line("@a", 3, 17, "1(", "7)", 0.123456789) == "@a\t3\t17\t1(\t7)\t0.123457\n"


def test_parser_options():
    a = cli.build_parser().parse_args(["scan", "-f", "x.fq", "-q", "m.txt", "--out1", "a.raw", "--out-stems", "s.txt", "--out-stem-pairs", "p.txt",
                                       "--stem-min-prob", "0.2", "--logo-min-exist", "0.5"])
    assert (a.out_stems, a.out_stem_pairs, a.stem_min_prob, a.logo_min_exist) == ("s.txt", "p.txt", 0.2, 0.5)
    a = cli.build_parser().parse_args(["scan", "-f", "x.fq", "-q", "m.txt", "--out1", "a.raw"])
    assert a.out_stems is None and a.out_stem_pairs is None and a.stem_min_prob == 0.01


def test_sharded_writer_joins_the_counts_of_two_ranks_in_input_order_before_the_sum(tmp_path):
    recs = [("@r%d" % k, None, None) for k in range(5)]
    out1, outs = str(tmp_path / "scan.raw"), str(tmp_path / "stems.txt")
    rng = np.random.default_rng(9)
    slots = np.array([[0, 2], [1, 1]])
    counts = {rid: rng.random((2, 5, 5)) for rid, _, _ in recs}
    exist = {rid: 0.2 * k for k, (rid, _, _) in enumerate(recs)}

    def part(mine):
        for rid, _, _ in mine:
            yield "scan %s\n" % rid, io.stem_counts_record(rid, exist[rid], counts[rid])

    for rank in (1, 0):
        cli.sharded_write(recs, [out1, outs + ".seqs"], rank, 2, part, lambda: None)
    assert [rid for rid, _, _ in io.read_stem_counts(outs + ".seqs")] == ["@r%d" % k for k in range(5)]
    cli.write_stems_from_parts(outs + ".seqs", outs, "z.o", slots, 0.4)
    back = io.read_stems(outs)
    assert (back["n_used"], back["n_total"]) == (3, 5)
    want = np.zeros((2, 5, 5))
    for k in (2, 3, 4):                                                      # (input order)
        want += counts["@r%d" % k]
    assert np.array_equal(back["counts"], want)
    assert sorted(p.name for p in tmp_path.iterdir()) == ["scan.raw", "stems.txt"]


def test_stem_symbols_are_declared_and_exported():
    declared = set(re.findall(r"\b(elemdp_[a-z_0-9]+)\s*\(", open(HEADER).read()))
    lib = api.load_library()
    for name in ("elemdp_stem_slots", "elemdp_stem_profile", "elemdp_stem_list"):
        assert name in declared and name in api.SYMBOLS and hasattr(lib, name)
    assert hasattr(api.Engine, "stem_slots") and hasattr(api.Engine, "stem_profiles") and callable(api.stem_logo)


def test_the_slots_need_no_device_and_equal_the_drivers():
    eng = api.Engine(P1, PAR, 50, 30, 1e-4, 0.1, 0, 0)
    slots = eng.stem_slots()
    assert slots.tolist() == [[0, 0], [0, 8], [1, 7], [2, 6], [4, 4], [8, 8]]
    assert np.array_equal(slots, sc.StemDriver(P1, PAR).slots)
    i32 = C.POINTER(C.c_int32)
    buf = np.zeros(8, dtype=np.int32)
    assert api.load_library().elemdp_stem_slots(eng._h, buf.ctypes.data_as(i32), buf.ctypes.data_as(i32), 3) == -1    # ELEMDP_EINVAL
    for pattern in ("(.....)", "(.*)", ".(.*)."):
        assert np.array_equal(api.Engine(pattern, PAR, 50, 30, 1e-4, 0.1, 0, 0).stem_slots(), sc.StemDriver(pattern, PAR).slots)


@pytest.mark.skipif(have_gpu(), reason="only meaningful on a machine without a GPU")
def test_a_call_without_a_device_is_refused():
    eng = api.Engine(P1, PAR, 50, 30, 1e-4, 0.1, 0, 0)
    x = np.zeros(eng.n_param)
    out = np.zeros(25 * len(eng.stem_slots()))
    dp, i32 = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    lib = api.load_library()
    assert lib.elemdp_stem_profile(eng._h, x.ctypes.data_as(dp), eng.n_param, 0.0, out.ctypes.data_as(dp), None) == -2     # ELEMDP_ENODEV
    assert lib.elemdp_stem_list(eng._h, None, None, None, None, None, 0) == -2
