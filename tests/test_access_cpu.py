"""Accessibility on the CPU: the four path sums of access_rules.h over the oracle's tables
(access_check.table_access) against brute-force enumeration with the oracle (access_check.enumerated_access); the product rule
through the test-only CPU driver (tests/access_emul.cpp), both forms, against both references; the identities with the pair
posteriors and between the widths; the edges; the record format, the parser, the sharded writer and the symbol."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from oracle import pyoracle as po
from rnaelem_amd import api, cli, io, synth
from tests import access_check as ac
from tests import ctx_check as cc
from tests.pair_check import oracle_pairs
from tests.test_host_abi import have_gpu
from tests.test_pair_posterior_gpu import PAR, perturbed
from tests.util import REPO

HEADER = os.path.join(REPO, "include", "elemdp.h")
PATTERNS = ["((.*.))", "(.*)", "(.....)"]
LENGTHS = (12, 15, 18, 20)         # (synth seed 100 + L)
U = 6
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
    """(x, seqs, quals, enumerated, (table accessibility, its terms)) of a case, computed once"""
    if case not in _refs:
        pattern, flags, min_bpp = case
        x, seqs, quals = case_inputs(case)
        o = ac.access_oracle(pattern, 50, 30, min_bpp=min_bpp, flags=flags)
        o.set_params(x)
        enum = [ac.enumerated_access(o, s, q, U) for s, q in zip(seqs, quals)]
        tab = [ac.table_access(o, s, q, x, U) for s, q in zip(seqs, quals)]
        _refs[case] = (x, seqs, quals, enum, tab)
    return _refs[case]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%s-%d-%g" % c)
def test_table_path_sums_equal_the_enumeration(case):
    x, seqs, quals, enum, tab = references(case)
    assert sum(e is not None for e in enum) >= 3
    for k, (e, t) in enumerate(zip(enum, tab)):
        assert (e is None) == (t is None), k
        if e is not None:
            ac.assert_access(t[0], e, what=(case, k))


def test_both_multi_loop_terms_are_covered_by_the_cases():
    """with energies the two multi-loop terms are ~1e-8 and the absolute tolerance would hide a wrong one: some case without
    energies must carry each of them at 1e-3 or more, in the reference"""
    top = {k: 0.0 for k in ac.TERMS}
    for case in CASES:
        for t in references(case)[4]:
            if t is not None:
                for k in ac.TERMS:
                    top[k] = max(top[k], float(t[1][k].max()))
    assert top["2"] >= 1e-3 and top["M"] >= 1e-3 and top["L"] >= 1e-3 and top["O"] >= 1e-3, top


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%s-%d-%g" % c)
def test_product_rule_on_the_cpu_equals_both_references(case):
    """access_rules.h through the CPU driver: the scaled-linear form over the compact tables of the product's CPU sweeps (plain and
    table-driven unary phases) and the log-space form over the dense ones"""
    pattern, flags, min_bpp = case
    x, seqs, quals, enum, tab = references(case)
    drv = ac.AccessDriver(pattern, PAR, 50, 30, min_bpp, 0.1, flags)
    for fast in (False, True):
        drv.set_fast(fast)
        for k, (s, q) in enumerate(zip(seqs, quals)):
            for form in (ac.AccessDriver.LIN, ac.AccessDriver.LOG):
                got, terms, used = drv.access(x, s, q, U, form)
                if enum[k] is None:
                    assert used == ac.AccessDriver.LOG and np.array_equal(got, ac.all_ones(len(s), U), equal_nan=True), (case, k)
                    continue
                assert used == form, (case, k, form)
                ac.assert_access(got, enum[k], what=(case, k, form, "enumerated"))
                ac.assert_access(got, tab[k][0], what=(case, k, form, "tables"))
                valid = ~ac.nan_tail(len(s), U)
                for name in ac.TERMS:
                    np.testing.assert_allclose(terms[name][valid], tab[k][1][name][valid], rtol=1e-8, atol=1e-10,
                                               err_msg=str((case, k, form, name)))


@pytest.mark.parametrize("flags", [0, po.NO_ENE], ids=["energies", "no_ene"])
def test_product_rule_at_a_narrow_band_equals_the_tables(flags):
    """W = 20 at L = 5, 19, 20, 21, 47: tails behind a branch that sits as the right part of a bifurcation, which the
    scaled-linear form reads from the pair table of the factorised rule 2"""
    pattern, W, Uw = "((.*.))", 20, 8
    x = perturbed(api.Engine(pattern, PAR, W, 30, 1e-4, 0.1, flags, 0))
    o = ac.access_oracle(pattern, W, 30, flags=flags)
    o.set_params(x)
    drv = ac.AccessDriver(pattern, PAR, W, 30, 1e-4, 0.1, flags)
    top2 = 0.0
    for L in (5, 19, 20, 21, 47):
        (s,), (q,) = synth.synth_batch(1, L, seed=100 + L)
        ref, rterms = ac.table_access(o, s, q, x, Uw)
        top2 = max(top2, float(rterms["2"].max()))
        valid = ~ac.nan_tail(L, Uw)
        for fast in (False, True):
            drv.set_fast(fast)
            for form in (0, 1):
                got, terms, used = drv.access(x, s, q, Uw, form)
                assert used == form
                ac.assert_access(got, ref, what=(flags, L, fast, form))
                np.testing.assert_allclose(terms["2"][valid], rterms["2"][valid], rtol=1e-8, atol=1e-12, err_msg=str((flags, L, fast, form)))
    if flags:
        assert top2 >= 1e-3, top2


@pytest.mark.parametrize("pattern", PATTERNS)
def test_width_one_is_the_unpaired_vector_and_wider_windows_are_rarer(pattern):
    x = perturbed(api.Engine(pattern, PAR, 50, 30, 1e-4, 0.1, 0, 0))
    o = ac.access_oracle(pattern, 50, 30)
    o.set_params(x)
    drv = ac.AccessDriver(pattern, PAR, 50, 30, 1e-4, 0.1, 0)
    for L in (18, 40, 71):
        (s,), (q,) = synth.synth_batch(1, L, seed=100 + L)
        P = oracle_pairs(o, s, q)
        assert P is not None
        paired = np.zeros(L)
        for i in range(L + 1):
            for d in range(1, P.shape[1]):
                if i + d <= L and P[i, d] != 0.0:
                    paired[i] += P[i, d]
                    paired[i + d - 1] += P[i, d]
        for form in (0, 1):
            got, _, _ = drv.access(x, s, q, U, form)
            np.testing.assert_allclose(got[:, 0], 1.0 - paired, rtol=0, atol=1e-12, err_msg=str((pattern, L, form)))
            for w in range(1, U):
                n = L - w          # windows of width w + 1
                assert np.all(got[:n, w] <= np.minimum(got[:n, w - 1], got[1:n + 1, w - 1]) + 1e-12), (pattern, L, form, w)


@pytest.mark.parametrize("L", [1, 2, 4])
def test_nan_exactly_where_the_window_runs_off_the_end(L):
    pattern = "((.*.))"
    x = perturbed(api.Engine(pattern, PAR, 50, 30, 1e-4, 0.1, 0, 0))
    drv = ac.AccessDriver(pattern, PAR)
    s = np.arange(L, dtype=np.uint8) % 4 + 1
    q = np.full(L + 1, 10, dtype=np.uint8)
    for form in (0, 1):
        got, _, _ = drv.access(x, s, q, U, form)
        ac.assert_access(got, ac.all_ones(L, U), what=(L, form), rtol=0, atol=1e-12)     # (no pair fits: every base is exterior)


def test_sequences_without_a_parse_and_models_without_structure_are_exactly_one():
    pattern = "((.*.))"
    o = ac.access_oracle(pattern)
    x, seqs, quals = cc.no_parse_inputs(perturbed(api.Engine(pattern, PAR, 50, 30, 1e-4, 0.1, 0, 0)), o.hmm())
    o.set_params(x)
    assert ac.table_access(o, seqs[0], quals[0], x, U) is None
    ref = ac.table_access(o, seqs[1], quals[1], x, U)[0]
    drv = ac.AccessDriver(pattern, PAR)
    for form in (0, 1):
        got, _, used = drv.access(x, seqs[0], quals[0], U, form)
        assert used == ac.AccessDriver.LOG and np.array_equal(got, ac.all_ones(len(seqs[0]), U), equal_nan=True)
        ac.assert_access(drv.access(x, seqs[1], quals[1], U, form)[0], ref, what=form)
    m = io.read_model(os.path.join(REPO, "tests", "golden", "2.model"))
    assert m["no_rss"]
    drv = ac.AccessDriver(m["pattern"], m["ene_param"], m["max_span"], m["max_iloop"], m["min_bpp"], m["tau"], m["flags"])
    (s,), (q,) = synth.synth_batch(1, 40, seed=3)
    for form in (0, 1):
        assert np.array_equal(drv.access(m["x"], s, q, U, form)[0], ac.all_ones(40, U), equal_nan=True)


def test_record_round_trip(tmp_path):
    rng = np.random.default_rng(1)
    accs = []
    for L in (1, 9, 30):
        a = rng.random((L, 5))
        a[ac.nan_tail(L, 5)] = np.nan
        accs.append(a)
    accs[1][3, 2] = 0.0
    path = tmp_path / "access.txt"
    path.write_text("".join(io.access_record("@s%d extra words" % k, a) for k, a in enumerate(accs)))
    back = io.read_access_records(str(path))
    assert [rid for rid, _ in back] == ["@s%d extra words" % k for k in range(3)]
    for (_, b), a in zip(back, accs):
        assert b.shape == a.shape and np.array_equal(np.isnan(b), np.isnan(a))
        np.testing.assert_allclose(b, a, rtol=5e-6, atol=0)
    text = io.access_record("@a", accs[0])
    assert text.split("\n")[0] == "id: @a" and [l.split(": ")[0] for l in text.split("\n")[1:6]] == ["u%d" % w for w in range(1, 6)]
    assert text.split("\n")[1] == "u1: [%.6g]" % accs[0][0, 0] and text.split("\n")[2] == "u2: [nan]"


def test_parser_options():
    a = cli.build_parser().parse_args(["scan", "-f", "x.fq", "-q", "m.txt", "--out1", "a.raw", "--out-access", "u.txt", "--access-width", "8"])
    assert (a.out_access, a.access_width) == ("u.txt", 8)
    a = cli.build_parser().parse_args(["scan", "-f", "x.fq", "-q", "m.txt", "--out1", "a.raw"])
    assert a.out_access is None and a.access_width == 16


def test_sharded_writer_joins_the_access_parts_of_two_ranks_in_input_order(tmp_path):
    recs = [("@r%d" % k, None, None) for k in range(5)]
    out1, outa = str(tmp_path / "scan.raw"), str(tmp_path / "access.txt")
    acc = ac.all_ones(3, 2) * 0.5

    def part(mine):
        for rid, _, _ in mine:
            yield "scan %s\n" % rid, io.access_record(rid, acc)

    for rank in (1, 0):
        cli.sharded_write(recs, [out1, outa], rank, 2, part, lambda: None)
    assert open(out1).read() == "".join("scan @r%d\n" % k for k in range(5))
    assert [rid for rid, _ in io.read_access_records(outa)] == ["@r%d" % k for k in range(5)]
    assert sorted(p.name for p in tmp_path.iterdir()) == ["access.txt", "scan.raw"]


def test_access_symbol_is_declared_and_exported():
    declared = set(re.findall(r"\b(elemdp_[a-z_0-9]+)\s*\(", open(HEADER).read()))
    assert "elemdp_accessibility" in declared and "elemdp_accessibility" in api.SYMBOLS
    assert hasattr(api.load_library(), "elemdp_accessibility")
    assert hasattr(api.Engine, "accessibility")


@pytest.mark.skipif(have_gpu(), reason="only meaningful on a machine without a GPU")
def test_a_call_without_a_device_is_refused():
    eng = api.Engine("((.*.))", PAR, 50, 30, 1e-4, 0.1, 0, 0)
    x = np.zeros(eng.n_param)
    out = np.zeros(16)
    dp = C.POINTER(C.c_double)
    assert api.load_library().elemdp_accessibility(eng._h, x.ctypes.data_as(dp), eng.n_param, 16, out.ctypes.data_as(dp)) == -2     # ELEMDP_ENODEV
