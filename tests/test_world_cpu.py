"""Scan posteriors in one world on the CPU: the references of tests/world_check.py against each other on the
twelve tiny cases of tests/test_ctx_cpu.py; the sampler's walk in a world through the test-only CPU driver
(tests/world_sample_emul.cpp) against the oracle; the option -- its values, its round trip through the Python methods, the record of
options a streamed batch replays --; the command line and the `# world:` line; the refusal without a device."""
import ctypes as C
import os

import numpy as np
import pytest

from rnaelem_amd import api, cli
from tests import cond_check as cd
from tests import ctx_check as cc
from tests import world_check as wc
from tests.test_cond_cpu import motif_heavy
from tests.test_ctx_cpu import CASES, case_inputs
from tests.test_host_abi import have_gpu
from tests.test_pair_posterior_gpu import PAR, perturbed
from tests.test_pair_shapes_gpu import P1, batch
from tests.util import REPO

HEADER = os.path.join(REPO, "include", "elemdp.h")
TABLE_PRODUCTS = ("pairs", "context", "nodes", "access", "loops")
_refs = {}


def references(case):
    """(x, seqs, quals, enumerated worlds, table worlds) of a tiny case, computed once"""
    if case not in _refs:
        pattern, flags, min_bpp = case
        x, seqs, quals = case_inputs(case)
        o = cc.ctx_oracle(pattern, 50, 30, min_bpp=min_bpp, flags=flags)
        o.set_params(x)
        on = cc.ctx_oracle(pattern, 50, 30, min_bpp=min_bpp, flags=flags)
        xn = cd.none_params(x, o.hmm())
        enum = [wc.enumerated_worlds(o, s, q) for s, q in zip(seqs, quals)]
        tab = [wc.table_worlds(o, on, x, xn, s, q, TABLE_PRODUCTS) for s, q in zip(seqs, quals)]
        _refs[case] = (x, seqs, quals, enum, tab)
    return _refs[case]


# ---- 1. references 2 and 3 against each other

@pytest.mark.parametrize("case", CASES, ids=lambda c: "%s-%d-%g" % c)
def test_the_tables_of_both_worlds_equal_the_enumeration(case):
    x, seqs, quals, enum, tab = references(case)
    assert all(t["e"] >= wc.E_MIN for t in tab), [t["e"] for t in tab]      # (reference 2 holds for every sequence of the batch)
    assert "nodes" in enum[0]["motif"]      # (the node rows of L = 12 can be enumerated under every pattern)
    for k, (e, t) in enumerate(zip(enum, tab)):
        assert np.isfinite(e["Zari"]) and np.isfinite(e["Znasi"]), k
        for w in wc.WORLDS:
            wc.assert_world(e[w], t, w, what=(case, k))
        # the mixture of the enumerated worlds is the mixture's tables reference
        for p in TABLE_PRODUCTS:
            if p not in e["motif"]:
                continue
            np.testing.assert_allclose(e["e"] * e["motif"][p] + (1.0 - e["e"]) * e["none"][p], t["mixed"][p], rtol=1e-8, atol=wc.ATOL[p],
                                       equal_nan=True, err_msg=str((case, k, p)))


def test_the_worlds_differ_in_the_tiny_cases():
    """a swap of the worlds, or the mixture in place of a world, cannot pass: somewhere the context letters and the node profile of
    the two worlds differ by a lot, and the world without the motif puts every base on node 0"""
    dc = dn = 0.0
    for case in CASES:
        for e in references(case)[3]:
            dc = max(dc, np.abs(e["motif"]["context"] - e["none"]["context"]).max())
            if "nodes" in e["motif"]:
                dn = max(dn, np.abs(e["motif"]["nodes"] - e["none"]["nodes"]).max())
                assert np.all(e["none"]["nodes"][:, 0] == 1.0)
    assert dc > 0.1 and dn > 0.5, (dc, dn)


# ---- 2. the sampler in a world

@pytest.mark.parametrize("fast", [False, True], ids=["plain", "table-driven"])
def test_the_sampler_walks_one_world(fast):
    """L = 5, 20, 47 at W = 20 (L = 5 is shorter than the pattern's body: an empty motif world): status, logp against the weight of
    the derivation relative to Z_w, the nodes of each world; the draw numbering is the mixture's -- a sample whose mixture draw fell
    into the world is the same sample in the world"""
    seqs, quals = batch((5, 20, 47), seed=77, neg_every=0)
    eng = api.Engine(P1, PAR, 20, 30, 1e-4, 0.1, 0, 0)
    o = cc.ctx_oracle(P1, 20, 30)
    x = motif_heavy(perturbed(eng), o.hmm(), by=1.0)
    o.set_params(x)
    drv = wc.WorldDriver(P1, PAR, 20, 30, 1e-4, 0.1, 0)
    wc.driver().emu_set_fast(drv.h, int(fast))
    M = eng.n_node
    n_distinct = dict(motif=0, none=0)
    for k, (s, q) in enumerate(zip(seqs, quals)):
        mixed = drv.sample(x, s, q, 50, 11, k, 0)
        in_motif = ((mixed[1] != 0) & (mixed[1] != M - 1)).any(axis=1)
        for w, world in ((1, "motif"), (2, "none")):
            got = drv.sample(x, s, q, 50, 11, k, w)
            n_distinct[world] += wc.check_samples(o, s, q, got, world, M, what=(fast, k, world))
            if got[3] == 0:
                same = in_motif if world == "motif" else ~in_motif
                for t in np.nonzero(same)[0]:
                    assert got[0][t] == mixed[0][t] and np.array_equal(got[1][t], mixed[1][t]), (k, world, t)
        t = o.train_seq(s, q)
        assert np.isfinite(t["Zari"]) == (len(s) > 5), (k, t["Zari"])
    assert n_distinct["motif"] > 10 and n_distinct["none"] > 10, n_distinct


# ---- 3. the option

def test_world_takes_0_1_2_and_refuses_anything_else():
    eng = api.Engine(P1)
    lib = api.load_library()
    for v in (0, 1, 2, 0):
        assert lib.elemdp_set_option(eng._h, b"world", float(v)) == 0
    for v in (3, -1, 0.5, float("nan")):
        assert lib.elemdp_set_option(eng._h, b"world", float(v)) == -1, v      # ELEMDP_EINVAL
        assert b"world" in lib.elemdp_last_error()
    assert api.world_index("mixed") == 0 and api.world_index("motif") == 1 and api.world_index("none") == 2 and api.world_index(2) == 2
    for bad in ("both", 3, -1, None, True):
        with pytest.raises(ValueError):
            api.world_index(bad)


WORLD_METHODS = ("pair_posteriors", "mea_structures", "sample_structures", "context_profiles", "node_profiles", "joint_profiles",
                 "stem_profiles", "helix_posteriors", "loop_posteriors", "accessibility", "mea_alignments")


def test_the_python_methods_set_the_world_and_put_it_back(monkeypatch):
    """every listed method takes world=, sets the option for the call and restores the previous value, also when the call raises
    (here it raises in every case: no batch is loaded, or there is no device)"""
    eng = api.Engine(P1)
    assert eng.world == "mixed"
    seen = []
    real = api.Engine.set_option

    def spy(self, key, value):
        seen.append((key, int(value)))
        real(self, key, value)

    monkeypatch.setattr(api.Engine, "set_option", spy)
    x = np.zeros(eng.n_param)
    for before in ("mixed", "none"):
        eng.set_option("world", api.world_index(before))
        for name in WORLD_METHODS:
            args = (x, 5) if name == "sample_structures" else (x,)
            del seen[:]
            with pytest.raises((api.ElemdpError, TypeError, AttributeError)):
                getattr(eng, name)(*args, world="motif")
            assert seen == [("world", 1), ("world", api.world_index(before))], (name, seen)
            assert eng.world == before
            del seen[:]
            with pytest.raises((api.ElemdpError, TypeError, AttributeError)):
                getattr(eng, name)(*args, world=before)      # (the world it is in already: nothing to set)
            assert seen == [] and eng.world == before
            with pytest.raises(ValueError):
                getattr(eng, name)(*args, world="both")
    assert not hasattr(api.Engine.scan, "__wrapped__") and not hasattr(api.Engine.conditional_pairs, "__wrapped__")
    assert not hasattr(api.Engine.train_eval, "__wrapped__")


def test_setting_the_world_again_replaces_its_entry_in_the_option_record():
    """the record of options the inner engines of a streamed batch replay (elemdp_last_timing entry 5) takes one entry for world,
    however often it is set; any other option still appends"""
    eng = api.Engine(P1)
    n0 = eng.options_logged()
    eng.set_option("world", 1)
    assert eng.options_logged() == n0 + 1
    for k in range(200):
        eng.set_option("world", k % 3)
    assert eng.options_logged() == n0 + 1
    eng.set_option("fast", 0)
    eng.set_option("world", 2)
    eng.set_option("fast", 1)
    assert eng.options_logged() == n0 + 3
    with pytest.raises(api.ElemdpError):
        eng.set_option("world", 7)
    assert eng.options_logged() == n0 + 3 and eng.world == "none"


# ---- 4. the command line

def test_scan_parser_takes_the_world():
    base = ["scan", "-f", "a.fq", "-q", "m.txt", "--out1", "a.raw"]
    assert cli.build_parser().parse_args(base).world == "mixed"
    for w in ("mixed", "motif", "none"):
        assert cli.build_parser().parse_args(base + ["--world", w]).world == w
    with pytest.raises(SystemExit):
        cli.build_parser().parse_args(base + ["--world", "both"])
    assert (cli.world_header("mixed"), cli.world_header("motif"), cli.world_header("none")) == ("", "# world: motif\n", "# world: none\n")


@pytest.mark.parametrize("ranks", [1, 2])
def test_a_product_file_of_a_world_starts_with_its_line_and_is_otherwise_unchanged(tmp_path, ranks):
    recs = [("@r%d" % k, None, None) for k in range(5)]

    def part(mine):
        for rid, _, _ in mine:
            yield "scan %s\n" % rid, "context %s\n" % rid

    def write(d, headers):
        os.makedirs(str(tmp_path / d))
        outs = [str(tmp_path / d / "scan.raw"), str(tmp_path / d / "context.txt")]
        for rank in reversed(range(ranks)):
            cli.sharded_write(recs, outs, rank, ranks, part, lambda: None, headers)
        assert sorted(p.name for p in (tmp_path / d).iterdir()) == ["context.txt", "scan.raw"]
        return [open(o).read() for o in outs]

    plain = write("mixed", None)
    assert write("mixed2", ["", cli.world_header("mixed")]) == plain
    got = write("motif", ["", cli.world_header("motif")])
    assert got[0] == plain[0] and got[1] == "# world: motif\n" + plain[1]


# ---- 5. the header, and no device

def test_the_header_states_the_option():
    text = open(HEADER).read()
    doc = text.split('"world"', 1)[1].split("measurement / tests", 1)[0]
    for call in ("elemdp_pair_posteriors", "elemdp_pair_mea", "elemdp_sample", "elemdp_context_profile", "elemdp_node_profile",
                 "elemdp_node_mea", "elemdp_joint_profile", "elemdp_stem_profile", "elemdp_helix_posteriors", "elemdp_loop_posteriors",
                 "elemdp_accessibility"):
        assert call in doc.split("Ignored by")[0], call
    for call in ("elemdp_scan", "elemdp_pair_conditional", "train calls"):
        assert call in doc.split("Ignored by")[1], call
    assert "ELEMDP_EINVAL" in doc and "empty" in doc


@pytest.mark.skipif(have_gpu(), reason="only meaningful on a machine without a GPU")
def test_every_call_in_a_world_refuses_to_run_without_a_gpu():
    eng = api.Engine(P1)
    x = np.zeros(eng.n_param)
    # (no batch can be loaded without a device: offsets of one sequence of 8 bases, so that the wrappers reach the library)
    eng._off, eng._qoff, eng.n_seq = np.array([0, 8], dtype=np.int32), np.array([0, 9], dtype=np.int32), 1
    for w in ("motif", "none"):
        for name in WORLD_METHODS:
            args = (x, 5) if name == "sample_structures" else (x,)
            with pytest.raises(api.ElemdpError) as err:
                getattr(eng, name)(*args, world=w)
            assert err.value.code == -2, (name, err.value)      # ELEMDP_ENODEV
            assert eng.world == "mixed"
    dp = C.POINTER(C.c_double)
    lib = api.load_library()
    eng.set_option("world", 1)
    m = C.c_int64()
    assert lib.elemdp_pair_posteriors(eng._h, x.ctypes.data_as(dp), eng.n_param, 0.0, C.byref(m), None) == -2
    prof = np.zeros(8)
    assert lib.elemdp_context_profile(eng._h, x.ctypes.data_as(dp), eng.n_param, prof.ctypes.data_as(dp)) == -2
    assert lib.elemdp_accessibility(eng._h, x.ctypes.data_as(dp), eng.n_param, 4, prof.ctypes.data_as(dp)) == -2
