"""Helix posteriors on the CPU: the references of tests/helix_check.py against each other (enumeration with
the oracle, the definition in numpy over the oracle's tables); the product rule through the test-only CPU driver
(tests/helix_emul.cpp), both forms and both unary forms, against them; the three properties; the stems of a dot-bracket string; the
files; the symbols."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from oracle import pyoracle as po
from rnaelem_amd import api, io, synth
from tests import helix_check as hc
from tests import pair_check as pc
from tests.test_host_abi import have_gpu
from tests.util import REPO

HEADER = os.path.join(REPO, "include", "elemdp.h")
PAR = hc.PAR
P1, P5 = "((.*.))", "(.....)"
LENS = tuple(range(1, 61))
_shape = {}

# every test of this file belongs to the helix call: without its symbols the module does not import
assert all(name in api.SYMBOLS for name in ("elemdp_helix_posteriors", "elemdp_helix_list"))


def shape_reference(pattern, W, L):
    """(x, seq, qual, oracle, table H) of a shape case, computed once"""
    if (pattern, W, L) not in _shape:
        eng = api.Engine(pattern, PAR, W, 30, 1e-4, 0.1, 0, 0)
        x = hc.helix_params(eng)
        o = hc.helix_oracle(pattern, W, 30)
        o.set_params(x)
        (s,), (q,) = synth.synth_batch(1, L, seed=300 + L)
        _shape[(pattern, W, L)] = (x, s, q, o, hc.table_helices(o, s, q, x, kmax=10))
    return _shape[(pattern, W, L)]


@pytest.mark.parametrize("case", hc.CASES, ids=hc.case_id)
def test_references_agree_on_the_enumerated_cases(case):
    """the definition over the tables equals the enumeration, which knows nothing of rules: no 0 x 0 interior loop joins two
    stacked pairs outside rule 1b"""
    x, s, q, o, enum = hc.tiny_reference(case)
    assert enum is not None
    hc.assert_helix(hc.table_helices(o, s, q, x), enum, what=case)


def test_the_enumerated_cases_hold_helices_of_three_pairs():
    """conditions on the reference, with room over the values seen (0.604, 0.461, 0.136): with energies every pattern has an entry
    with k >= 3 above 0.01 in at least one case; (.*) at L = 16 reaches k = 4; the joint probability of the best helix of
    ((.*.)) at 14 bases is well below its best pair's (0.859 against 0.604)"""
    best = {}
    for case in hc.CASES:
        enum = hc.tiny_reference(case)[4]
        assert enum[:, :, 1].max() > 0.01, case
        if not case[2] & po.NO_ENE:
            best[case[0]] = max(best.get(case[0], 0.0), enum[:, :, 2:].max())
    assert len(best) == 3 and all(v > 0.1 for v in best.values()), best
    deep = hc.tiny_reference(("(.*)", 16, po.NO_ENE, 0.0))[4]
    assert deep[:, :, 3].max() > 1e-3 and not deep[:, :, 4:].any()
    pat = hc.tiny_reference(("((.*.))", 14, 0, 1e-4))[4]
    assert pat[:, :, 0].max() - 0.2 > pat[:, :, 2].max() > 0.3


@pytest.mark.parametrize("case", hc.CASES, ids=hc.case_id)
def test_product_rule_on_the_cpu_equals_the_enumeration(case):
    """helix_rules.h through the CPU driver: the scaled-linear form over the compact tables of the product's CPU sweeps (plain and
    table-driven unary phases) and the log-space form over the dense ones; H(., 1) is the P of the pair reference"""
    pattern, _, flags, min_bpp = case
    x, s, q, o, enum = hc.tiny_reference(case)
    drv = hc.HelixDriver(pattern, PAR, 50, 30, min_bpp, 0.1, flags)
    P = pc.oracle_pairs(o, s, q)
    L = len(s)
    for fast in (False, True):
        drv.set_fast(fast)
        for form in (hc.HelixDriver.LIN, hc.HelixDriver.LOG):
            got, _, used = drv.helices(x, s, q, form)
            assert used == form, (case, form)
            hc.assert_helix(got, enum, what=(case, fast, form))
            assert got.min() >= 0.0 and got.max() <= 1.0
            hc.assert_properties(got, 1e-12 if form == 0 else 1e-10, what=(case, fast, form))
            for i in range(L):
                for d in range(1, min(P.shape[1] - 1, L - i) + 1):
                    assert got[i, i + d, 0] == pytest.approx(P[i, d], rel=1e-8, abs=1e-10), (case, fast, form, i, d)


@pytest.mark.parametrize("pattern", [P1, P5])
def test_product_rule_on_the_cpu_at_many_lengths(pattern):
    """L = 1 .. 60 at W = 20: the driver against the table definition, both forms; the three properties"""
    drv = hc.HelixDriver(pattern, PAR, 20, 30, 1e-4, 0.1, 0)
    top = 0.0
    for L in LENS:
        x, s, q, o, ref = shape_reference(pattern, 20, L)
        for form in (hc.HelixDriver.LIN, hc.HelixDriver.LOG):
            got, _, used = drv.helices(x, s, q, form, kmax=10)
            if ref is None:
                assert not got.any(), (pattern, L)
                continue
            assert used == form
            hc.assert_helix(got, ref, what=(pattern, L, form))
            hc.assert_properties(got, 1e-12 if form == 0 else 1e-10, what=(pattern, L, form))
            top = max(top, got[:, :, 2].max())
    assert top > 0.05, top


def test_thresholds_and_stems_of_the_driver():
    """the exact pruning of the stop rule: with min_prob > 0 a chain keeps the lengths at or above it and nothing else; a stem's
    probability is the chain's value at its length, whatever the length, and 0 where a pair is not kept"""
    x, s, q, o, ref = shape_reference(P1, 20, 47)
    drv = hc.HelixDriver(P1, PAR, 20, 30, 1e-4, 0.1, 0)
    full, _, _ = drv.helices(x, s, q, 0, kmax=10)
    cut, _, _ = drv.helices(x, s, q, 0, kmax=10, min_prob=0.02)
    assert np.array_equal(cut, np.where(full >= 0.02, full, 0.0)) and 0 < (cut > 0).sum() < (full > 0).sum()
    ii, jj, kk = np.nonzero(full)
    stems = [(int(i), int(j), int(k) + 1) for i, j, k in zip(ii, jj, kk)][::7]
    _, kept, _, _ = o.bpp(s)
    lost = next((i, i + d, 1) for i in range(len(s)) for d in range(5, 20) if i + d <= len(s) and not kept[i, d])
    _, sp, _ = drv.helices(x, s, q, 0, kmax=10, stems=stems + [lost, (0, len(s), 1)])
    assert np.array_equal(sp[:-2], [full[i, j, k - 1] for i, j, k in stems]) and sp[-2] == 0.0 and sp[-1] == 0.0


def test_structure_helices():
    assert api.structure_helices("") == []
    assert api.structure_helices("....") == []
    assert api.structure_helices("((...))") == [(0, 7, 2)]
    assert api.structure_helices("((.(...)))") == [(0, 10, 2), (3, 8, 1)]                       # bulged: two stems
    assert api.structure_helices("(((...)).)") == [(0, 10, 1), (1, 8, 2)]
    assert api.structure_helices(".((..))(...).") == [(1, 7, 2), (7, 12, 1)]                    # side by side
    assert api.structure_helices("((..)(..))") == [(0, 10, 1), (1, 5, 1), (5, 9, 1)]            # a multi-loop right inside a pair
    assert api.structure_helices("()") == [(0, 2, 1)]
    for bad in ("(", ")", "(()", "())", ")(", "(.x.)", "[..]"):
        with pytest.raises(ValueError):
            api.structure_helices(bad)


def test_files_round_trip(tmp_path):
    rows = [("seq one", 0, 9, 2, 0.75), ("seq one", 0, 9, 3, 0.5), ("b", 4, 30, 2, 1.25e-3)]
    text = "".join(io.helix_line(rid, i + 1, j, n, p) for rid, i, j, n, p in rows)
    f = tmp_path / "h.txt"
    f.write_text(text)
    got = io.read_helices(str(f))
    assert [(r["id"], r["i"], r["j"], r["len"]) for r in got] == [(rid, i, j, n) for rid, i, j, n, _ in rows]
    np.testing.assert_allclose([r["p"] for r in got], [r[4] for r in rows], rtol=1e-5)
    mrows = [("a", 2, 20, 4, 0.4, 0.6), ("c d", 0, 7, 1, 0.0, 0.0)]
    g = tmp_path / "m.txt"
    g.write_text("".join(io.mea_helix_line(rid, i + 1, j, n, p, pm) for rid, i, j, n, p, pm in mrows))
    got = io.read_mea_helices(str(g))
    assert [(r["id"], r["i"], r["j"], r["len"]) for r in got] == [(rid, i, j, n) for rid, i, j, n, _, _ in mrows]
    np.testing.assert_allclose([(r["p"], r["p_min"]) for r in got], [r[4:] for r in mrows], rtol=1e-5)
    for bad, reader in (("a\t1\t2\t3\n", io.read_helices), ("a\t1\t2\t3\t0.5\n", io.read_mea_helices)):
        f.write_text(bad)
        with pytest.raises(ValueError):
            reader(str(f))
    pairs = (np.array([0, 1, 2, 7]), np.array([12, 11, 10, 9]), np.array([0.9, 0.4, 0.7, 0.2]), None)
    assert api.stem_min_posterior(pairs, 0, 12, 3) == 0.4 and api.stem_min_posterior(pairs, 0, 12, 4) == 0.0


def test_header_declares_the_calls_and_the_bound():
    text = open(HEADER).read()
    assert re.search(r"#define\s+ELEMDP_HELIX_MAX_LEN\s+32\b", text) and api.HELIX_MAX_LEN == 32
    for name in ("elemdp_helix_posteriors", "elemdp_helix_list"):
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name


@pytest.mark.skipif(have_gpu(), reason="only meaningful on a machine without a GPU")
def test_a_call_without_a_device_is_refused():
    eng = api.Engine(P1, PAR, 50, 30, 1e-4, 0.1, 0, 0)
    x = np.zeros(eng.n_param)
    lib = api.load_library()
    assert lib.elemdp_helix_posteriors(eng._h, x.ctypes.data_as(C.POINTER(C.c_double)), eng.n_param, 16, 2, 0.0, None, None, None, None) == -2   # ELEMDP_ENODEV
    assert lib.elemdp_helix_list(eng._h, None, None, None, None, None, 0) == -2
