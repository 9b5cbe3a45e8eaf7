"""Hard structure constraints on the CPU: the mask rule of constraint_rules.h through the host entry
elemdp_constraint_mask_host against the brute force of constraint_check.apply; every refusal with its message; the reader of the
constraint file, the parser, the header line of the sharded writer, the symbols, and the refusal without a device."""
import ctypes as C
import re

import numpy as np
import pytest

from rnaelem_amd import api, cli, io, synth
from tests import constraint_check as kc
from tests.test_host_abi import have_gpu
from tests.util import REPO
import os

HEADER = os.path.join(REPO, "include", "elemdp.h")
PAR = "~T2004~"
SHAPES = [(1, 20), (5, 20), (12, 20), (33, 20), (47, 20), (107, 50)]     # (L, max_span): (L+1)(W+1) is and is not a multiple of 32


def sequence(L, seed=None):
    (s,), _ = synth.synth_batch(1, L, seed=100 + L if seed is None else seed)
    return s


def filter_mask(rng, seq, L, W, keep=0.6, min_span=5):
    """a stand-in for the filter's result: a random part of the canonical pairs"""
    kept = np.zeros((L + 1, W + 1), dtype=np.uint8)
    for i in range(L):
        for d in range(min_span, W + 1):
            if i + d <= L and kc.canonical(seq, L, W, min_span, i, i + d - 1) and rng.random() < keep:
                kept[i, d] = 1
    return kept


def both(kept, seq, cons, W):
    L = len(seq)
    ref = kc.apply(kept, seq, cons, L, W)
    got = api.constraint_mask_host(kept, seq, cons)
    assert np.array_equal(got[0], ref[0]), (cons, np.argwhere(got[0] != ref[0])[:5])
    assert np.array_equal(got[1], ref[1]), cons
    return got


def first_pair(seq, L, W, lo=0, hi=None, min_d=5):
    hi = L if hi is None else hi
    for i in range(lo, hi):
        for j in range(i + min_d - 1, min(hi, i + W)):
            if kc.canonical(seq, L, W, 5, i, j):
                return i, j
    raise AssertionError("no canonical pair")


def with_chars(L, chars):
    c = ["."] * L
    for p, ch in chars.items():
        c[p] = ch
    return "".join(c)


def test_all_free_returns_the_mask_unchanged_and_unp_all_ones():
    rng = np.random.default_rng(0)
    for L, span in SHAPES:
        W = min(L, span)
        s = sequence(L)
        kept = filter_mask(rng, s, L, W)
        out, unp = both(kept, s, "." * L, W)
        assert np.array_equal(out, kept) and unp.all() and len(unp) == L + 1


@pytest.mark.parametrize("ch", list("x|<>"))
def test_every_single_base_character_alone(ch):
    L, W = 33, 20
    s = sequence(L)
    kept = filter_mask(np.random.default_rng(1), s, L, W, keep=1.0)
    for p in (0, 7, 16, L - 1):
        out, unp = both(kept, s, with_chars(L, {p: ch}), W)
        assert unp[p] == (1 if ch == "x" else 0) and unp.sum() == L + (1 if ch == "x" else 0)
        opens = out[p, 1:].sum()
        closes = sum(out[p - d + 1, d] for d in range(1, W + 1) if p - d + 1 >= 0)
        if ch == "x":
            assert opens == 0 and closes == 0
        if ch == "<":
            assert closes == 0 and opens == kept[p, 1:].sum()
        if ch == ">":
            assert opens == 0
        if ch == "|":
            assert opens == kept[p, 1:].sum()
        # the cells that do not touch p stay
        touch = np.zeros_like(kept, dtype=bool)
        touch[p, :] = True
        for d in range(1, W + 1):
            if p - d + 1 >= 0:
                touch[p - d + 1, d] = True
        assert np.array_equal(out[~touch], kept[~touch])


def test_one_forced_pair_drops_its_rivals_and_every_crossing_pair():
    L, W = 47, 20
    s = sequence(L)
    kept = filter_mask(np.random.default_rng(2), s, L, W, keep=1.0)
    a, b = first_pair(s, L, W, lo=10, min_d=9)
    out, unp = both(kept, s, with_chars(L, {a: "(", b: ")"}), W)
    assert out[a, b - a + 1] == 1 and out[a, 1:].sum() == 1 and unp[a] == 0 and unp[b] == 0
    for i in range(L):
        for d in range(1, W + 1):
            if out[i, d]:
                r = i + d - 1
                assert not (a < i < b < r) and not (i < a < r < b)
    assert out.sum() < kept.sum()


def test_nested_adjacent_and_enclosing_forced_pairs():
    L, W = 107, 50
    s = sequence(L)
    kept = filter_mask(np.random.default_rng(3), s, L, W)
    a, b = first_pair(s, L, W, lo=5, hi=60, min_d=30)
    c, d = first_pair(s, L, W, lo=a + 1, hi=b, min_d=5)              # nested in (a, b)
    e, f = first_pair(s, L, W, lo=b + 1, hi=L, min_d=5)              # adjacent, behind (a, b)
    for chars in ({a: "(", b: ")", c: "(", d: ")"}, {a: "(", b: ")", e: "(", f: ")"}, {a: "(", b: ")", c: "(", d: ")", e: "(", f: ")"},
                  {a: "(", b: ")", c: "(", d: ")", c + 1: "x", c + 2: "|", e: "<"}):
        both(kept, s, with_chars(L, chars), W)
    if d + 1 < b and c - 1 > a:      # directly stacked: ((...))
        both(kept, s, with_chars(L, {a: "(", a + 1: "<", b: ")"}), W)


def test_a_forced_pair_the_filter_dropped_comes_back():
    L, W = 33, 20
    s = sequence(L)
    a, b = first_pair(s, L, W, lo=3)
    kept = filter_mask(np.random.default_rng(4), s, L, W)
    kept[a, b - a + 1] = 0
    out, _ = both(kept, s, with_chars(L, {a: "(", b: ")"}), W)
    assert out[a, b - a + 1] == 1
    out, _ = both(np.zeros_like(kept), s, with_chars(L, {a: "(", b: ")"}), W)
    assert out.sum() == 1


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "L%d-W%d" % s)
def test_random_strings_equal_the_brute_force(shape):
    L, span = shape
    W = min(L, span)
    n_forced = 0
    for seed in range(20):
        rng = np.random.default_rng(1000 * L + seed)
        s = sequence(L, seed=seed + 7)
        kept = filter_mask(rng, s, L, W)
        cons = kc.random_string(rng, s, L, W)
        n_forced += cons.count("(")
        both(kept, s, cons, W)
    assert n_forced > 0 or L < 12


def refused(kept, seq, cons):
    with pytest.raises(api.ElemdpError) as e:
        api.constraint_mask_host(kept, seq, cons)
    assert e.value.code == -1          # ELEMDP_EINVAL
    return str(e.value)


def test_every_refusal_names_what_is_wrong():
    L, W = 33, 20
    s = sequence(L)
    kept = filter_mask(np.random.default_rng(5), s, L, W)
    a, b = first_pair(s, L, W)
    assert "unbalanced" in refused(kept, s, with_chars(L, {a: "("})) and "position %d" % a in refused(kept, s, with_chars(L, {a: "("}))
    assert "unbalanced" in refused(kept, s, with_chars(L, {b: ")"}))
    assert "unknown character 'y' at position 4" in refused(kept, s, with_chars(L, {4: "y"}))
    assert "characters for a sequence of %d" % L in refused(kept, s, "." * (L - 1))
    assert "characters for a sequence of %d" % L in refused(kept, s, "." * (L + 1))
    # not a pairing combination, too short a span, wider than the band: each names sequence, i and j
    i, j = next((i, j) for i in range(L) for j in range(i + 4, min(L, i + W)) if (int(s[i]), int(s[j])) not in kc.PAIRING)
    msg = refused(kept, s, with_chars(L, {i: "(", j: ")"}))
    assert "sequence 0" in msg and "bases %d and %d" % (i, j) in msg and "canonical" in msg
    i, j = next((i, j) for i in range(L) for j in (i + 2,) if j < L and (int(s[i]), int(s[j])) in kc.PAIRING)
    assert "bases %d and %d" % (i, j) in refused(kept, s, with_chars(L, {i: "(", j: ")"}))
    i, j = next((i, j) for i in range(L) for j in range(i + W, L) if (int(s[i]), int(s[j])) in kc.PAIRING)
    assert "bases %d and %d" % (i, j) in refused(kept, s, with_chars(L, {i: "(", j: ")"}))
    # the brute force refuses the same strings
    for cons in (with_chars(L, {a: "("}), with_chars(L, {4: "y"}), with_chars(L, {i: "(", j: ")"})):
        with pytest.raises(ValueError):
            kc.apply(kept, s, cons, L, W)
    lib = api.load_library()
    assert lib.elemdp_constraint_mask_host(None, None, b"..", 2, 2, 0, None, None) == -1


def test_satisfies_agrees_with_the_mask_on_enumerated_structures():
    """the two references against each other: every structure over the constrained mask that satisfies the string is one over
    the filter's mask plus the forced pairs, and a structure over the filter's mask that satisfies the string has all its pairs
    in the constrained mask"""
    from tests import ctx_check as cc
    L, W = 16, 16
    s = io.encode_seq("GGGACUUCGGUCCCAG")
    kept = filter_mask(np.random.default_rng(6), s, L, W, keep=1.0)
    dbs = cc.structures(kept, L, W)
    for cons in ("...x....x.......", "|...............", "(............)..", ".x(...xx...)|...", "..<.........>...", "((..........)).x"):
        out, _ = kc.apply(kept, s, cons, L, W)
        want = sorted(db for db in dbs if kc.satisfies(db, cons))
        got = sorted(db for db in cc.structures(out, L, W) if kc.satisfies(db, cons))
        assert got == want and 0 < len(want) < len(dbs), cons


# ---- plumbing --------------------------------------------------------------------------------------------------------------------

def test_check_constraints_fills_free_entries_and_refuses_wrong_shapes():
    assert api.check_constraints([None, "x.|"], [2, 3]) == ["..", "x.|"]
    with pytest.raises(ValueError, match="2 characters for a sequence of 3"):
        api.check_constraints(["..", ".."], [2, 3])
    with pytest.raises(ValueError, match="1 constraint strings for 2 sequences"):
        api.check_constraints([".."], [2, 3])


def test_constraint_file_reader(tmp_path):
    p = tmp_path / "c.txt"
    p.write_text(">s1 some words\n..((..\n..))..\n\n>s3\nxx|\n")
    cons = io.read_constraints(str(p))
    assert cons == {"s1": "..((....))..", "s3": "xx|"}
    recs = [("@s1 a b", np.zeros(12, dtype=np.uint8), None), ("@s2", np.zeros(4, dtype=np.uint8), None), ("@s3", np.zeros(3, dtype=np.uint8), None)]
    assert io.constraints_for(recs, cons) == ["..((....))..", None, "xx|"]
    with pytest.raises(ValueError, match="no FASTQ record is named 's3'"):
        io.constraints_for(recs[:2], cons)
    recs[2] = ("@s3", np.zeros(5, dtype=np.uint8), None)
    with pytest.raises(ValueError, match="'s3' has 3 characters, the sequence 5 bases"):
        io.constraints_for(recs, cons)
    with pytest.raises(SystemExit, match="--constraints: .*'s3' has 3 characters"):
        cli.read_constraints_for(recs, str(p))
    assert cli.read_constraints_for(recs, None) is None
    p.write_text("..\n>a\n..\n")
    with pytest.raises(ValueError, match="before the first"):
        io.read_constraints(str(p))
    p.write_text(">a\n..\n>a\n..\n")
    with pytest.raises(ValueError, match="given twice"):
        io.read_constraints(str(p))


def test_parser_options():
    a = cli.build_parser().parse_args(["scan", "-f", "x.fq", "-q", "m.txt", "--out1", "a.raw", "--constraints", "c.txt", "--chunk", "7"])
    assert a.constraints == "c.txt" and a.chunk == 7
    a = cli.build_parser().parse_args(["eval", "-f", "x.fq", "-q", "m.txt", "--out1", "a", "--out2", "b", "--constraints", "c.txt"])
    assert a.constraints == "c.txt"
    assert cli.build_parser().parse_args(["scan", "-f", "x.fq", "-q", "m.txt", "--out1", "a.raw"]).constraints is None
    with pytest.raises(SystemExit):
        cli.build_parser().parse_args(["train", "-f", "x.fq", "-m", "(.*)", "--out1", "m", "--constraints", "c.txt"])


@pytest.mark.parametrize("world", [1, 2])
def test_product_files_start_with_the_constraints_line(tmp_path, world):
    recs = [("@r%d" % k, None, None) for k in range(5)]
    out1, outp = str(tmp_path / "scan.raw"), str(tmp_path / "pairs.txt")
    head = cli.constraints_header("c.txt") + cli.world_header("motif")
    assert head == "# constraints: c.txt\n# world: motif\n" and cli.constraints_header(None) == ""

    def part(mine):
        for rid, _, _ in mine:
            yield "scan %s\n" % rid, "pairs %s\n" % rid

    for rank in reversed(range(world)):
        cli.sharded_write(recs, [out1, outp], rank, world, part, lambda: None, ["", head])
    assert open(out1).read() == "".join("scan @r%d\n" % k for k in range(5))
    assert open(outp).read() == head + "".join("pairs @r%d\n" % k for k in range(5))
    assert sorted(p.name for p in tmp_path.iterdir()) == ["pairs.txt", "scan.raw"]


def test_symbols_are_declared_and_exported():
    declared = set(re.findall(r"\b(elemdp_[a-z_0-9]+)\s*\(", open(HEADER).read()))
    lib = api.load_library()
    for sym in ("elemdp_load_batch_constrained", "elemdp_constraint_mask_host"):
        assert sym in declared and sym in api.SYMBOLS and hasattr(lib, sym)
    assert lib.elemdp_abi_version() == 1


@pytest.mark.skipif(have_gpu(), reason="only meaningful on a machine without a GPU")
def test_a_constrained_load_without_a_device_is_refused():
    eng = api.Engine("((.*.))", PAR, 50, 30, 1e-4, 0.1, 0, 0)
    seqs, quals = synth.synth_batch(2, 12)
    with pytest.raises(api.ElemdpError) as e:
        eng.load_batch(seqs, quals, constraints=["x" * 12, None])
    assert e.value.code == -2          # ELEMDP_ENODEV


# ---- the product rules on the CPU under a constraint against the enumeration -----------------------------------------------------------

@pytest.fixture(scope="module")
def enum_cases():
    return kc.enumerated_cases()


def test_every_enumerated_case_keeps_and_drops_structures(enum_cases):
    unsat = []
    for case, _, _, _, refs in enum_cases:
        for c, e in refs:
            if e["n_sat"] == 0:
                unsat.append(c)
            else:
                assert e["n_sat"] >= 2 and e["n_dropped"] >= 2, (case, c)
    assert unsat == ["..........|........."]          # the one unsatisfiable string: it must give no parse


@pytest.mark.parametrize("fast", [0, 1])
def test_product_rules_on_the_cpu_equal_the_enumeration(fast, enum_cases):
    """tests/constraint_emul.cpp: the host rule on the plan of prepare(), plan_finish() with the structure imposed, the sweeps of
    the scan's first sum pass in both forms, then ln Z_c, P, unpaired and the seven context letters"""
    from tests import ctx_check as cc
    from tests.util import assert_log_close
    n_fast = 0
    for case, x, s, q, refs in enum_cases:
        pattern, L, flags, min_bpp = case
        drv = kc.ConstraintDriver(pattern, PAR, 50, 30, min_bpp, 0.1, flags)
        drv.set_fast(fast)
        for c, e in refs:
            for form in (kc.ConstraintDriver.LIN, kc.ConstraintDriver.LOG):
                got = drv.run(x, s, q, c, form)
                what = (case, c, fast, form)
                if not np.isfinite(e["lnZ"]):
                    assert np.isneginf(got["lnZ"]) and got["form"] == kc.ConstraintDriver.LOG, what
                    assert np.all(got["P"] == 0.0) and np.all(got["unpaired"] == 1.0), what
                    assert np.array_equal(got["ctx"], cc.exterior_only(L)), what
                    continue
                assert got["form"] == form, what
                assert_log_close(got["lnZ"], e["lnZ"], what=str(what))
                np.testing.assert_allclose(got["P"], e["P"], rtol=1e-8, atol=1e-12, err_msg=str(what))
                np.testing.assert_allclose(got["unpaired"], e["unpaired"], rtol=1e-8, atol=1e-10, err_msg=str(what))
                cc.assert_profile(got["ctx"], e["ctx"], what=what)


def test_the_fix_rss_table_reference_of_a_whole_structure_equals_the_enumeration(enum_cases):
    """what tests/test_constraint_gpu.py compares the node profile of a whole structure with at L = 47 and 107 --
    node_check.table_profile on an oracle made with DBG_FIX_RSS, through constraint_check.FixedOracle -- against the enumeration
    over node rows for one structure of a tiny case"""
    from oracle import pyoracle as po
    from tests import ctx_check as cc
    from tests import joint_check as jc
    from tests import node_check as nc
    case, x, s, q, refs = enum_cases[0]
    pattern, L, flags, min_bpp = case
    o = jc.joint_oracle(pattern, 50, 30, min_bpp=min_bpp, flags=flags)
    o.set_params(x)
    db = max(refs[0][1]["dbs"], key=lambda d: o.derivation_logz(s, q, d, None))
    assert "(" in db
    e = dict(lnZ=o.derivation_logz(s, q, db, None), dbs=[db])
    kc.node_reference(o, s, q, e, kc.live_rows(o, s, q))
    of = cc.ctx_oracle(pattern, 50, 30, min_bpp=min_bpp, flags=flags | po.DBG_FIX_RSS)
    nc.assert_profile(nc.table_profile(kc.FixedOracle(of, db, 50), s, q, x), e["node"], cols=range(e["node"].shape[1]))


def test_the_cpu_driver_refuses_what_the_load_refuses():
    s = io.encode_seq("GGGACUUCGGUCCCAG")
    drv = kc.ConstraintDriver("(.*)", PAR, 50, 30, 0.0, 0.1, 0)
    x = np.zeros(api.Engine("(.*)", PAR, 50, 30, 0.0, 0.1, 0, 0).n_param)
    with pytest.raises(RuntimeError, match="bases 1 and 9 cannot be forced"):
        drv.run(x, s, np.full(17, 10, dtype=np.uint8), ".(.......)......")          # G - G
