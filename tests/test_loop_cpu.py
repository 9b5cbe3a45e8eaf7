"""Loop posteriors on the CPU: the references of tests/loop_check.py against each other (enumeration with the
oracle, the definitions in numpy over the oracle's tables); the product rule through the test-only CPU driver
(tests/loop_emul.cpp), both forms and both unary forms, against them; the identities with the pair, helix and context rules; the
threshold; the loops of a dot-bracket string; the files; the symbols."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from oracle import pyoracle as po
from rnaelem_amd import api, io, synth
from tests import loop_check as lc
from tests.test_host_abi import have_gpu
from tests.util import REPO

HEADER = os.path.join(REPO, "include", "elemdp.h")
PAR = lc.PAR
P1, P5 = "((.*.))", "(.....)"
LENS = tuple(range(1, 61))
_shape = {}

# every test of this file belongs to the loop call: without its symbols the module does not import
assert all(name in api.SYMBOLS for name in ("elemdp_loop_posteriors", "elemdp_loop_closing_list", "elemdp_loop_two_list"))


def shape_reference(pattern, W, L):
    """(x, seq, qual, oracle, table reference) of a shape case, computed once"""
    if (pattern, W, L) not in _shape:
        eng = api.Engine(pattern, PAR, W, 30, 1e-4, 0.1, 0, 0)
        x = lc.loop_params(eng)
        o = lc.loop_oracle(pattern, W, 30)
        o.set_params(x)
        (s,), (q,) = synth.synth_batch(1, L, seed=300 + L)
        _shape[(pattern, W, L)] = (x, s, q, o, lc.table_loops(o, s, q, x))
    return _shape[(pattern, W, L)]


@pytest.mark.parametrize("case", lc.CASES, ids=lc.case_id)
def test_references_agree_on_the_enumerated_cases(case):
    """the definitions over the tables equal the enumeration, which knows nothing of rules"""
    x, s, q, o, enum = lc.tiny_reference(case)
    assert enum is not None
    cols, two, _ = lc.table_loops(o, s, q, x)
    lc.assert_loop(cols, enum[0], what=case)
    lc.assert_two(two, enum[1], what=case)


def test_the_enumerated_cases_hold_every_kind_of_loop():
    """conditions on the reference itself, with room under the values seen (H 0.609, S 0.854, B 0.122, I 0.246, two-loop 0.13 on
    .(.*). at 13 bases; M 0.0149 at (.*), 16 and 0.0366 at (.*), 18 without energies -- with energies M is ~1e-9): every column
    has weight somewhere, and without energies one 14-base case alone holds every kind of loop but the multi-branch one"""
    best = np.zeros(5)
    top_two = 0.0
    for case in lc.CASES:
        cols, two = lc.tiny_reference(case)[4]
        best = np.maximum(best, cols.reshape(-1, 5).max(axis=0))
        top_two = max([top_two] + list(two.values()))
    assert best[lc.H_] > 0.5 and best[lc.S_] > 0.7 and best[lc.B_] > 0.1 and best[lc.I_] > 0.2 and best[lc.M_] > 0.01, best
    assert top_two > 0.1
    assert lc.tiny_reference(("(.*)", 16, po.NO_ENE, 0.0))[4][0][:, :, lc.M_].max() > 0.01
    cols = lc.tiny_reference(("(.*)", 14, po.NO_ENE, 0.0))[4][0]
    assert (cols.reshape(-1, 5).max(axis=0)[:4] > 0.05).all()          # (seen on this one case: 0.205, 0.061, 0.122, 0.127)


@pytest.mark.parametrize("case", lc.CASES, ids=lc.case_id)
def test_product_rule_on_the_cpu_equals_the_enumeration(case):
    """loop_rules.h through the CPU driver: the scaled-linear form over the compact tables of the product's CPU sweeps (plain and
    table-driven unary phases) and the log-space form over the dense ones; the identities of the five columns and the two-loops
    with P, H(., 2) and the context profile of the same tables"""
    pattern, _, flags, min_bpp = case
    x, s, q, o, enum = lc.tiny_reference(case)
    drv = lc.LoopDriver(pattern, PAR, 50, 30, min_bpp, 0.1, flags)
    for fast in (False, True):
        drv.set_fast(fast)
        for form in (lc.LoopDriver.LIN, lc.LoopDriver.LOG):
            r = drv.loops(x, s, q, form)
            assert r["form"] == form, (case, form)
            lc.assert_loop(r["cols"], enum[0], what=(case, fast, form))
            lc.assert_two(r["two"], enum[1], what=(case, fast, form))
            assert r["cols"].min() >= 0.0 and r["cols"].max() <= 1.0
            lc.assert_identities(len(s), r["cols"], r["P"], r["two"], r["h2"], r["profile"], 1e-12 if form == 0 else 1e-10,
                                 what=(case, fast, form))


@pytest.mark.parametrize("pattern", [P1, P5])
def test_product_rule_on_the_cpu_at_many_lengths(pattern):
    """L = 1 .. 60 at W = 20: the driver against the table definitions, both forms; the identities"""
    drv = lc.LoopDriver(pattern, PAR, 20, 30, 1e-4, 0.1, 0)
    top = np.zeros(5)
    for L in LENS:
        x, s, q, o, ref = shape_reference(pattern, 20, L)
        for form in (lc.LoopDriver.LIN, lc.LoopDriver.LOG):
            r = drv.loops(x, s, q, form)
            if ref is None:
                assert not r["cols"].any() and not r["two"], (pattern, L)
                continue
            assert r["form"] == form
            lc.assert_loop(r["cols"], ref[0], what=(pattern, L, form))
            lc.assert_two(r["two"], ref[1], what=(pattern, L, form))
            lc.assert_loop(r["P"], ref[2], what=(pattern, L, form, "P"))
            lc.assert_identities(L, r["cols"], r["P"], r["two"], r["h2"], r["profile"], 1e-12 if form == 0 else 1e-10,
                                 what=(pattern, L, form))
            top = np.maximum(top, r["cols"].reshape(-1, 5).max(axis=0))
    assert (top[:4] > 0.05).all(), top


def test_threshold_and_loops_of_the_driver():
    """with min_prob > 0 the walk covers the cells whose P reaches the pick bound and the two-loop list keeps exactly the entries
    of the full list at or above it, in its order; a loop of a structure has the value of the columns or of the list, bit for bit,
    and 0 exactly where a pair is not kept, a span exceeds the band, or a two-loop is no item"""
    x, s, q, o, ref = shape_reference(P1, 20, 47)
    drv = lc.LoopDriver(P1, PAR, 20, 30, 1e-4, 0.1, 0)
    full = drv.loops(x, s, q, 0)
    cut = drv.loops(x, s, q, 0, min_prob=0.02)
    keep = full["P"] >= 0.02
    assert np.array_equal(cut["cols"], np.where(keep[:, :, None], full["cols"], 0.0)) and 0 < keep.sum() < (full["P"] > 0).sum()
    assert list(cut["two"].items()) == [(k, v) for k, v in full["two"].items() if v >= 0.02] and 0 < len(cut["two"]) < len(full["two"])
    ii, jj, cc_ = np.nonzero(full["cols"][:, :, [lc.H_, lc.S_, lc.M_]])
    loops = [((1, 2, 5)[c], int(i), int(j), -1, -1) for i, j, c in zip(ii, jj, cc_)][::5]
    twos = [(3 if (k == i + 1) != (l == j - 1) else 4, i, j, k, l) for (i, j, k, l) in list(full["two"])[::7]]
    _, kept, _, _ = o.bpp(s)
    a, d = next((i, d) for i in range(len(s)) for d in range(5, 20) if i + d <= len(s) and not kept[i, d])
    (i0, j0, k0, l0) = next(iter(full["two"]))
    assert j0 - i0 > 7 and (i0, j0, i0 + 2, i0 + 4) not in full["two"]           # (a cell of two bases is never kept)
    lost = [(1, a, a + d, -1, -1), (2, 0, len(s), -1, -1), (4, i0, j0, i0 + 2, i0 + 4)]
    got = drv.loops(x, s, q, 0, loops=loops + twos + lost)["loops"]
    want = [full["cols"][i, j, t - 1] for t, i, j, _, _ in loops] + [full["two"][t[1:]] for t in twos]
    assert len(loops) > 3 and len(twos) > 3 and np.array_equal(got[:-3], want)
    assert list(got[-3:]) == [0.0, 0.0, 0.0]


def test_structure_loops():
    assert api.structure_loops("") == []
    assert api.structure_loops("....") == []
    assert api.structure_loops("((...))") == [(2, 0, 7, -1, -1), (1, 1, 6, -1, -1)]
    assert api.structure_loops("((.(...)))") == [(2, 0, 10, -1, -1), (3, 1, 9, 3, 8), (1, 3, 8, -1, -1)]              # a bulge on the left
    assert api.structure_loops("(((...)).)") == [(3, 0, 10, 1, 8), (2, 1, 8, -1, -1), (1, 2, 7, -1, -1)]              # on the right
    assert api.structure_loops("(.(...)..)") == [(4, 0, 10, 2, 7), (1, 2, 7, -1, -1)]                                  # an interior loop
    assert api.structure_loops(".((..))(...).") == [(2, 1, 7, -1, -1), (1, 2, 6, -1, -1), (1, 7, 12, -1, -1)]          # side by side
    assert api.structure_loops("((..)(..))") == [(5, 0, 10, -1, -1), (1, 1, 5, -1, -1), (1, 5, 9, -1, -1)]             # a multi-loop
    assert api.structure_loops("()") == [(1, 0, 2, -1, -1)]
    for db in ("((.(...)))", "(.(...)..)(((..)(..)))"):
        assert api.structure_loops(db) == lc.loops_of(db)
    for bad in ("(", ")", "(()", "())", ")(", "(.x.)", "[..]"):
        with pytest.raises(ValueError):
            api.structure_loops(bad)


def test_files_round_trip(tmp_path):
    closing = (np.array([0, 4]), np.array([20, 16]), np.array([0.9, 0.5]),
               np.array([[0.0, 0.5, 0.25, 0.125, 0.025], [0.5, 0.0, 0.0, 0.0, 0.0]]))
    two = (np.array([0, 0]), np.array([20, 20]), np.array([1, 3]), np.array([17, 18]), np.array([0.25, 0.125]))
    text = io.loop_lines("seq one", closing, two)
    assert text.count("\n") == 5 and [line.split("\t")[1] for line in text.split("\n")[:-1]] == ["S", "M", "B", "I", "H"]
    # a two-loop whose outer cell has no closing row keeps its place in (i, j) order and hides none behind it
    orphan = tuple(np.concatenate([c, v]) for c, v in zip(two, ([2, 5], [18, 15], [4, 6], [16, 14], [0.1, 0.2])))
    rows = [line.split("\t") for line in io.loop_lines("seq one", closing, orphan).split("\n")[:-1]]
    assert [(r[1], r[2], r[3]) for r in rows] == [("S", "1", "20"), ("M", "1", "20"), ("B", "1", "20"), ("I", "1", "20"),
                                                  ("I", "3", "18"), ("H", "5", "16"), ("I", "6", "15")]
    f = tmp_path / "l.txt"
    f.write_text(text)
    got = io.read_loops(str(f))
    assert [(r["id"], r["type"], r["i"], r["j"], r["k"], r["l"]) for r in got] == [
        ("seq one", "S", 0, 20, None, None), ("seq one", "M", 0, 20, None, None), ("seq one", "B", 0, 20, 1, 17),
        ("seq one", "I", 0, 20, 3, 18), ("seq one", "H", 4, 16, None, None)]
    np.testing.assert_allclose([r["p"] for r in got], [0.5, 0.025, 0.25, 0.125, 0.5], rtol=1e-5)
    g = tmp_path / "m.txt"
    g.write_text(io.mea_loop_line("a", "I", 3, 30, 6, 25, 0.4, 0.6) + io.mea_loop_line("c d", "H", 1, 7, None, None, 0.0, 0.0))
    got = io.read_mea_loops(str(g))
    assert [(r["id"], r["type"], r["i"], r["j"], r["k"], r["l"]) for r in got] == [("a", "I", 2, 30, 5, 25), ("c d", "H", 0, 7, None, None)]
    np.testing.assert_allclose([(r["p"], r["p_pair"]) for r in got], [(0.4, 0.6), (0.0, 0.0)], rtol=1e-5)
    for bad, reader in (("a\tH\t1\t2\t-\t-\n", io.read_loops), ("a\tH\t1\t2\t-\t-\t0.5\n", io.read_mea_loops),
                        ("a\tX\t1\t2\t-\t-\t0.5\n", io.read_loops), ("a\tB\t1\t2\t-\t-\t0.5\n", io.read_loops)):
        f.write_text(bad)
        with pytest.raises(ValueError):
            reader(str(f))


def test_header_declares_the_calls_and_the_types():
    text = open(HEADER).read()
    for t, letter in enumerate(api.LOOP_TYPES):
        if t:
            assert re.search(r"#define\s+ELEMDP_LOOP_%s\s+%d\b" % (letter, t), text), letter
    assert api.LOOP_TYPES[1:] == io.LOOP_LETTERS == lc.LETTERS
    for name in ("elemdp_loop_posteriors", "elemdp_loop_closing_list", "elemdp_loop_two_list"):
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name


@pytest.mark.skipif(have_gpu(), reason="only meaningful on a machine without a GPU")
def test_a_call_without_a_device_is_refused():
    eng = api.Engine(P1, PAR, 50, 30, 1e-4, 0.1, 0, 0)
    x = np.zeros(eng.n_param)
    lib = api.load_library()
    assert lib.elemdp_loop_posteriors(eng._h, x.ctypes.data_as(C.POINTER(C.c_double)), eng.n_param, 0.0, None, None, None, None, None,
                                      None) == -2   # ELEMDP_ENODEV
    assert lib.elemdp_loop_closing_list(eng._h, None, None, None, None, None, 0) == -2
    assert lib.elemdp_loop_two_list(eng._h, None, None, None, None, None, None, 0) == -2
