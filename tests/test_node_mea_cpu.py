"""Maximum expected accuracy motif alignments and site lists on the CPU: the two references of
tests/node_mea_check.py against each other, the product rule through the test-only CPU driver (tests/node_mea_emul.cpp) against
both, the chain lists against the rows of test_node_cpu, the stand-alone sanitizer build of the driver, the record format, the
parser and the symbol."""
import os
import re
import subprocess

import numpy as np
import pytest

from rnaelem_amd import api, cli, io, synth
from tests import ctx_check as cc
from tests import node_check as nc
from tests import node_mea_check as mc
from tests.test_node_cpu import CASES, P1, P2, node_params, tiny_reference
from tests.test_pair_posterior_gpu import PAR
from tests.test_pair_shapes_gpu import P2 as P2_LONG
from tests.util import REPO

HEADER = os.path.join(REPO, "include", "elemdp.h")
GAMMAS = (1.0, 4.0)
# (pattern, L, gamma, the first sites in order, the number of sites: exactly or at least)
MULTI = [("(...)", 16, 4.0, [(7, 14), (2, 7)], (2, 2)),
         ("...", 16, 1.0, [(7, 10), (4, 7), (10, 13)], (3, 4)),
         ("(.*.)", 15, 1.0, None, (1, 1))]
MULTI_K = 4
MARGIN = 1e-6
_multi = {}
_shape = {}


def names_of(pattern):
    return api.Engine(pattern, PAR, 50, 30, 1e-4, 0.1, 0, 0).describe()["node"]


def multi_reference(pattern, L):
    """(x, seq, qual, names, table profile) of a multi-site case, computed once"""
    if (pattern, L) not in _multi:
        eng = api.Engine(pattern, PAR, 50, 30, 1e-4, 0.1, 0, 0)
        x = node_params(eng)
        (s,), (q,) = synth.synth_batch(1, L, seed=100 + L)
        o = nc.node_oracle(pattern, 50, 30, min_bpp=1e-4)
        o.set_params(x)
        _multi[(pattern, L)] = (x, s, q, eng.describe()["node"], nc.table_profile(o, s, q, x))
    return _multi[(pattern, L)]


def tiny_names(case):
    return names_of(case[0])


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%s-%d-%d-%g" % c)
def test_tiny_cases_enumeration_chain_and_driver_agree(case):
    prof = tiny_reference(case)[4]
    names = tiny_names(case)
    for gamma in GAMMAS:
        brute = mc.brute_sites(prof, names, gamma, 1)
        assert all(b[3] >= MARGIN for b in brute), (case, gamma, [b[3] for b in brute])
        chain = mc.dp_sites(prof, names, gamma, 1)
        assert len(chain) == len(brute)
        for (rb, sb, vb, _), (rc, sc, vc) in zip(brute, chain):
            assert np.array_equal(rb, rc) and sb == sc and abs(vb - vc) <= 1e-12 * max(abs(vb), 1.0), (case, gamma)
        got = mc.driver_sites(prof, names, gamma, 1)
        mc.assert_equals_brute(got, brute, what=(case, gamma))
        mc.check_result(got, prof, names, gamma, 1, own_prof=prof, what=(case, gamma))


def test_the_tiny_cases_call_a_site_somewhere():
    called = 0
    for case in CASES:
        prof = tiny_reference(case)[4]
        called += len(mc.driver_sites(prof, tiny_names(case), 4.0, 1)["start"])
    assert called >= len(CASES) // 2, called


@pytest.mark.parametrize("pattern,L,gamma,sites,count", MULTI, ids=lambda v: str(v) if isinstance(v, (str, int, float)) else "")
def test_multi_site_cases(pattern, L, gamma, sites, count):
    x, s, q, names, prof = multi_reference(pattern, L)
    brute = mc.brute_sites(prof, names, gamma, MULTI_K)
    assert all(b[3] >= MARGIN for b in brute), (pattern, [b[3] for b in brute])
    found = [b[1] for b in brute if b[1] is not None]
    assert count[0] <= len(found) <= count[1], (pattern, found)
    if sites is not None:
        assert found[:len(sites)] == sites, (pattern, found)
    chain = mc.dp_sites(prof, names, gamma, MULTI_K)
    assert [c[1] for c in chain] == [b[1] for b in brute]
    for (rb, _, vb, _), (rc, _, vc) in zip(brute, chain):
        assert np.array_equal(rb, rc) and abs(vb - vc) <= 1e-12 * max(abs(vb), 1.0)
    got = mc.driver_sites(prof, names, gamma, MULTI_K)
    mc.assert_equals_brute(got, brute, what=pattern)
    mc.check_result(got, prof, names, gamma, MULTI_K, own_prof=prof, what=pattern)
    for a in range(len(found)):
        for b in range(a):
            assert found[a][1] <= found[b][0] or found[b][1] <= found[a][0]


def test_given_exclusions_bar_the_inner_nodes_only():
    x, s, q, names, prof = multi_reference("(...)", 16)
    free = mc.dp_sites(prof, names, 4.0, 1)[0]
    held = mc.dp_sites(prof, names, 4.0, 1, excluded=[free[1]])[0]
    assert held[1] == (2, 7) and held[2] < free[2]
    M = len(names)
    a, b = free[1]
    assert not ((held[0][a:b] > 0) & (held[0][a:b] < M - 1)).any()


def shape_profiles(pattern, W):
    """[(L, table profile or the no-parse profile)] at the lengths where something changes, computed once"""
    if (pattern, W) not in _shape:
        eng = api.Engine(pattern, PAR, W, 30, 1e-4, 0.1, 0, 0)
        x = node_params(eng)
        o = nc.node_oracle(pattern, W, 30)
        o.set_params(x)
        body = sum(c != "*" for c in pattern)
        out = []
        for L in (1, 2, body - 1, body, 49, 50, 51, 107):
            (s,), (q,) = synth.synth_batch(1, L, seed=300 + L)
            ref = nc.table_profile(o, s, q, x)
            out.append((L, ref if ref is not None else nc.no_parse_profile(L, eng.n_node)))
        _shape[(pattern, W)] = (eng.describe()["node"], out)
    return _shape[(pattern, W)]


@pytest.mark.parametrize("pattern,W", [(P1, 50), (P2, 50), (P2_LONG, 50), (P1, 20), (P2_LONG, 20)])
def test_driver_against_the_checker_at_many_lengths(pattern, W):
    names, profs = shape_profiles(pattern, W)
    sites = 0
    for L, prof in profs:
        for K in (1, 4):
            for gamma in GAMMAS:
                got = mc.driver_sites(prof, names, gamma, K)
                mc.check_result(got, prof, names, gamma, K, own_prof=prof, what=(pattern, W, L, K, gamma))
                sites += len(got["start"])
        one, four = mc.driver_sites(prof, names, 4.0, 1), mc.driver_sites(prof, names, 4.0, 4)
        assert np.array_equal(one["slots"]["rows"][0], four["slots"]["rows"][0])
    assert sites > 0


def test_a_sequence_without_any_parse_has_no_site():
    o = nc.node_oracle(P1)
    eng = api.Engine(P1, PAR, 50, 30, 1e-4, 0.1, 0, 0)
    x, seqs, quals = cc.no_parse_inputs(node_params(eng), o.hmm())
    o.set_params(x)
    assert nc.table_profile(o, seqs[0], quals[0], x) is None
    names = eng.describe()["node"]
    prof = nc.no_parse_profile(len(seqs[0]), eng.n_node)
    for K in (1, 4):
        got = mc.driver_sites(prof, names, 4.0, K)
        assert len(got["start"]) == 0
        mc.check_result(got, prof, names, 4.0, K, own_prof=prof)
    ref = nc.table_profile(o, seqs[1], quals[1], x)
    mc.check_result(mc.driver_sites(ref, names, 4.0, 4), ref, names, 4.0, 4, own_prof=ref)


def test_a_model_without_structure():
    path = os.path.join(REPO, "tests", "golden", "2.model")
    m = io.read_model(path)
    o, x = nc.node_oracle_from_model(path)
    names = "".join(o.hmm()["node"])
    for L in (3, 9, 40):
        (s,), (q,) = synth.synth_batch(1, L, seed=3)
        prof = nc.table_profile(o, s, q, x, tau=m["tau"])
        for K in (1, 4):
            for gamma in GAMMAS:
                mc.check_result(mc.driver_sites(prof, names, gamma, K), prof, names, gamma, K, own_prof=prof, what=(L, K, gamma))


def test_chain_lists_generate_the_alignment_rows():
    for names, L, want in (("z(.)o", 4, {"zzzz", "(.)o", "z(.)", "((.)", "(..)", "(.))"}), ("z.*o", 2, {"zz", ".o", "z.", "..", ".*"})):
        lo, first, last = mc.driver_lists(names)
        rows = {"".join(names[m] for m in r) for r in mc.rows_of_lists(lo, first, last, L)}
        assert rows == want, (names, rows)
        assert rows == {"".join(names[m] for m in r) for r in nc.alignments(L, names)}
        preds, f2, l2 = mc.chain_lists(names)
        assert [list(range(lo[m], m + 1)) for m in range(len(names))] == preds and list(first) == f2 and list(last) == l2
    for names in ("z((.*.))o", "z(.....)o", "z.*.*o", "z*.o", "z.**o"):
        lo, first, last = mc.driver_lists(names)
        for L in (1, 2, 5):
            assert mc.rows_of_lists(lo, first, last, L) == {tuple(int(v) for v in r) for r in nc.alignments(L, names)}, (names, L)
            assert all(mc.valid_row(r, names) for r in nc.alignments(L, names))


def test_valid_row_refuses_what_no_alignment_gives():
    names = "z(.)o"
    for bad in ([0, 4], [4, 4], [2, 3], [1, 2], [0, 1, 3], [1, 2, 3, 2], [5], []):
        assert not mc.valid_row(bad, names), bad
    assert mc.valid_row([0, 0], names) and mc.valid_row([1, 2, 3, 4], names) and mc.valid_row([0, 1, 2, 3], names)


def test_driver_refusals():
    prof = nc.no_parse_profile(4, 5)
    for gamma in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            mc.driver_sites(prof, "z(.)o", gamma, 1)
    for K in (0, 65):
        with pytest.raises(ValueError):
            mc.driver_sites(prof, "z(.)o", 1.0, K)


def test_stand_alone_driver_under_the_sanitizers(tmp_path):
    """node_mea_emul.cpp with its own main, address and undefined-behaviour sanitizers, no Python in the process: random profiles
    at L = 47 .. 107, K = 4"""
    exe = str(tmp_path / "node_mea_san")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-Wno-unknown-pragmas", "-DNODE_MEA_MAIN", "-o", exe, mc.SRC])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout


def test_site_record_round_trip(tmp_path):
    names = "z((.*.))o"
    rows = np.array([[0, 0, 1, 2, 3, 5, 6, 7, 8, 8], [1, 2, 3, 5, 6, 7, 8, 8, 8, 8]], dtype=np.uint8)
    res = [dict(rows=rows, start=np.array([2, 0]), end=np.array([8, 6]), score=np.array([9.25, 8.5]), confidence=np.array([0.75, 0.5])),
           dict(rows=np.zeros((0, 3), dtype=np.uint8), start=np.zeros(0, dtype=np.int32), end=np.zeros(0, dtype=np.int32),
                score=np.zeros(0), confidence=np.zeros(0))]
    path = tmp_path / "sites.txt"
    path.write_text("".join(io.site_record("@s%d extra words" % k, r, names) for k, r in enumerate(res)))
    back = io.read_sites(str(path))
    assert [b[0] for b in back] == ["@s0 extra words", "@s1 extra words"]
    for (_, got), want in zip(back, res):
        assert len(got["start"]) == len(want["start"])
        assert np.array_equal(got["start"], want["start"]) and np.array_equal(got["end"], want["end"])
        np.testing.assert_allclose(got["score"], want["score"], rtol=5e-6)
        np.testing.assert_allclose(got["confidence"], want["confidence"], rtol=5e-6)
        assert got["rows"] == ["".join(names[m] for m in r) for r in want["rows"]]
    lines = io.site_record("@a", res[0], names).split("\n")
    assert lines[0] == "id: @a" and lines[1] == "site 0: 2 8 9.25 0.75" and lines[2] == "zz((..))oo" and lines[5] == ""


def test_parser_options():
    a = cli.build_parser().parse_args(["scan", "-f", "x.fq", "-q", "m.txt", "--out1", "a.raw", "--out-sites", "s.txt"])
    assert (a.out_sites, a.site_gamma, a.max_sites) == ("s.txt", 1.0, 1)
    a = cli.build_parser().parse_args(["scan", "-f", "x.fq", "-q", "m.txt", "--out1", "a.raw", "--out-sites", "s.txt", "--site-gamma", "4",
                                       "--max-sites", "3"])
    assert (a.site_gamma, a.max_sites) == (4.0, 3)
    assert cli.build_parser().parse_args(["scan", "-f", "x.fq", "-q", "m.txt", "--out1", "a.raw"]).out_sites is None


def test_sharded_writer_joins_the_site_parts_of_two_ranks_in_input_order(tmp_path):
    recs = [("@r%d" % k, None, None) for k in range(5)]
    out1, outs = str(tmp_path / "scan.raw"), str(tmp_path / "sites.txt")
    res = dict(rows=np.array([[0, 1, 2]], dtype=np.uint8), start=np.array([1]), end=np.array([2]), score=np.array([2.5]),
               confidence=np.array([0.5]))

    def part(mine):
        for rid, _, _ in mine:
            yield "scan %s\n" % rid, io.site_record(rid, res, "z.o")

    for rank in (1, 0):
        cli.sharded_write(recs, [out1, outs], rank, 2, part, lambda: None)
    assert [rid for rid, _ in io.read_sites(outs)] == ["@r%d" % k for k in range(5)]


def test_node_mea_symbol_is_declared_and_exported():
    declared = set(re.findall(r"\b(elemdp_[a-z_0-9]+)\s*\(", open(HEADER).read()))
    assert "elemdp_node_mea" in declared and "elemdp_node_mea" in api.SYMBOLS
    assert hasattr(api.load_library(), "elemdp_node_mea")
    assert hasattr(api.Engine, "mea_alignments") and callable(io.site_record) and callable(io.read_sites)
