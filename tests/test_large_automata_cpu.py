"""The host side of the patterns of 63 to 130 interval states (tests/large_automata.py), without a GPU, so
that a failure of tests/test_large_automata_gpu.py points at a kernel: the state and node counts of the table, the automaton the
engine flattens (which patterns get the shadow copy of (0,0)), the automaton description against the oracle's, the rule headers
through the CPU emulation against the oracle (log-space, scaled-linear under the reference schedule and the merged one, pruned
and unpruned lists), the log-space rule headers of the posterior products through their CPU drivers against the table references,
the refusals, and -- from the oracle alone -- that the batches of the GPU file let the motif parse.

What the table-driven band programs fit (Emul.set_fast, bit 1; bit 4 for the automaton with the shadow state): with the pruned
lists, the engine's default, every accepted pattern of the table except S = 127; the launcher also wants the whole automaton
blob staged (at most 4096 ints), so of these the GPU file's train and scan cases run the table-driven forms at S = 63, 64 and
65 and the general band kernels from S = 78 (test_the_blob_is_staged_whole_up_to_65_states); with unpruned lists (option prune
0) none of the table fits.  No accepted pattern has more than 64 nodes (the largest is M = 43 at S = 127: a pair
node costs at least two states beside the loop states, and 128 states are reached first)."""
import numpy as np
import pytest

from oracle import pyoracle as po
from rnaelem_amd import api
from tests import cond_check as cd
from tests import large_automata as la
from tests.emul.pyemul import Emul
from tests.sample_check import oracle_map
from tests.test_pair_posterior_gpu import perturbed
from tests.util import assert_log_close

PAR = open(po.DEFAULT_PAR).read()
FAST_PRUNED = {63: 13, 64: 13, 65: 13, 78: 13, 126: 13, 127: 8, 128: 13}     # Emul.set_fast with the pruned lists
FAST_UNPRUNED = {63: 8, 64: 8, 65: 8, 78: 8, 126: 8, 127: 8, 128: 8}


def engine(S):
    return api.Engine(la.PATTERN[S], "~T2004~", 50, 30, 1e-4, 0.1, 0, 0)


def oracle_with(S, x):
    def make():
        o = po.make_oracle(la.PATTERN[S], 50, 30, min_bpp=1e-4, tau=0.1)
        o.set_params(x)
        return o
    return make


@pytest.mark.parametrize("S,M,pattern", la.TABLE, ids=[str(S) for S, _, _ in la.TABLE])
def test_state_and_node_counts_of_the_table(S, M, pattern):
    """a change to the automaton builder that moves a pattern across 64 or 128 states shows here"""
    e = Emul(pattern, PAR)
    assert (e.S, e.describe()["M"]) == (S, M)
    o = po.make_oracle(pattern, 50, 30)
    assert (o.hmm()["S"], o.hmm()["M"]) == (S, M)
    assert M <= 64          # (k_node_mea's second lane round, m += 64, is out of reach under the state limit)


@pytest.mark.parametrize("S,M,pattern", la.TABLE, ids=[str(S) for S, _, _ in la.TABLE])
def test_automaton_matches_the_oracle(S, M, pattern):
    got = Emul(pattern, PAR).describe()
    ref = po.make_oracle(pattern, 50, 30).hmm()
    for k in ("reg_pattern", "M", "S", "node", "theta_id", "theta_sizes", "state", "loop_state", "reachable", "right", "left",
              "pair", "loop_loop"):
        assert got[k] == ref[k], (pattern, k)


@pytest.mark.parametrize("S", la.ACCEPTED)
def test_the_engine_sweeps_the_shadow_state_below_127_states(S):
    """Engine::flatten_automaton appends the shadow copy of (0,0) for S < 127 only: a train evaluation then sweeps S + 1 <= 127
    active states under the merged schedule; S = 127 and 128 sweep the plain automaton under the reference's two outside passes.
    No handle sweeps more than 128 active states."""
    eng = engine(S)
    lay = eng.describe()["layout"]
    assert eng.describe()["S"] == S
    if S < la.SHADOW_BELOW:
        assert (lay["S"], lay["shadow"]) == (S + 1, S)
    else:
        assert (lay["S"], lay["shadow"]) == (S, -1)
    assert lay["S"] <= 128
    assert lay["fp_ok"] == (FAST_PRUNED[S] & (4 if S < la.SHADOW_BELOW else 1) != 0)


@pytest.mark.parametrize("S", la.ACCEPTED)
def test_the_blob_is_staged_whole_up_to_65_states(S):
    """Engine::prepare_lin stages the whole automaton blob in LDS up to 4096 ints (geometry_fast requires it): the band kernels
    run table-driven on S = 63, 64, 65 and in the general form, the blob in global memory, from S = 78"""
    assert (engine(S).describe()["layout"]["n_ints"] <= 4096) == (S <= 65)


@pytest.mark.parametrize("S", la.ACCEPTED)
def test_the_access_kernel_always_stages_its_automaton_blob(S):
    """launch_access_chains leaves the blob in global memory (n_ints = 0) once acc_lds_bytes exceeds 60 KiB: 8 (11 + n_theta) +
    4 * 8 (2 max(S, n_ap) + 2 U) + 4 n_small + 4 ((U + 7) & ~7) bytes.  With n_small <= n_ints (the whole blob) and the widest
    window of the suite, U = 64, no accepted pattern of the table comes near it: that form is out of reach under the state
    limit."""
    eng = engine(S)
    lay = eng.describe()["layout"]
    U = 64
    lds = 8 * (11 + eng.n_param - 2) + 32 * (2 * max(S, lay["n_ap"]) + 2 * U) + 4 * lay["n_ints"] + 4 * ((U + 7) & ~7)
    assert lds <= 60 * 1024, lds


@pytest.mark.parametrize("S,pattern", la.REFUSED, ids=[str(S) for S, _ in la.REFUSED])
def test_patterns_above_128_states_are_refused(S, pattern):
    assert Emul(pattern, PAR).S == S
    with pytest.raises(api.ElemdpError, match="more than 128 interval states") as e:
        api.Engine(pattern, "~T2004~", 50, 30, 1e-4, 0.1, 0, 0)
    assert e.value.code == -1


@pytest.mark.parametrize("S", la.ACCEPTED)
def test_which_patterns_fit_the_table_driven_programs(S):
    e = Emul(la.PATTERN[S], PAR)
    assert e.set_fast(True) == FAST_UNPRUNED[S]
    e.set_prune(True)
    assert e.set_fast(True) == FAST_PRUNED[S]


# ---- the rule headers against the oracle

EMUL_LENS = (57, 70)


@pytest.mark.parametrize("prune", [False, True], ids=["unpruned", "pruned"])
@pytest.mark.parametrize("S", la.ACCEPTED)
def test_emulated_rules_match_the_oracle(S, prune):
    """the comparisons of test_emul_vs_oracle.py (test_train_sequence_matches_oracle, test_linear_train_rules_match_oracle,
    test_pruned_train_rules_match_oracle) on two planted sequences under both labels: the log-space rules, the scaled-linear
    rules under the reference schedule (0) and under the merged sweep with the shadow state (2); with the pruned lists also
    through the table-driven programs where the pattern fits them"""
    seqs, quals = la.tc.relabelled(*la.mixed(EMUL_LENS, seed=500 + S))
    e = Emul(la.PATTERN[S], PAR)
    e.set_prune(prune)
    if prune:
        e.set_fast(True)
    x = perturbed(engine(S))
    o = oracle_with(S, x)()
    parsed = 0
    for seq, qual in zip(seqs, quals):
        a = o.train_seq(seq, qual)
        parsed += not a["skipped"]
        for linear in (None, 0, 2):
            b = e.train_seq(x, seq, qual, linear=linear)
            for k in ("Zo", "Zari", "Znasi"):
                assert_log_close(b[k], a[k], rtol=1e-11, what=(k, linear))
            if a["skipped"] or (linear == 2 and not np.isfinite(a["Znasi"])):
                continue
            assert b["skipped"] == 0
            assert b["f"] == pytest.approx(a["f"], rel=1e-10, abs=1e-12), linear
            for k in ("ENo", "ENx", "EHo", "EHx"):
                np.testing.assert_allclose(b[k], a[k], rtol=1e-9, atol=1e-11, err_msg=str((k, linear)))
    assert parsed >= 3


@pytest.mark.parametrize("S", la.SCAN)
def test_emulated_scan_matches_the_oracle(S):
    """test_scan_with_linear_sum_passes_matches_oracle / test_pruned_scan_matches_oracle on one planted sequence"""
    (seq,), (qual,) = la.mixed((70,), seed=600 + S)
    e = Emul(la.PATTERN[S], PAR)
    e.set_prune(True)
    x = perturbed(engine(S))
    a = oracle_with(S, x)().scan_seq(seq, qual)
    assert a["exist_prob"] > 0.0
    for linear in (False, True):
        b = e.scan_seq(x, seq, qual, linear=linear)
        assert (a["Ys"], a["Ye"]) == (b["Ys"], b["Ye"])
        for k in ("ZL", "ZeL", "PyNL"):
            assert_log_close(b[k], a[k], rtol=1e-10, atol=1e-10, what=k)
        for k in ("start", "end", "inner"):
            assert_log_close(b[k], a[k], rtol=1e-9, atol=1e-9, what=k)
        assert b["exist_prob"] == pytest.approx(a["exist_prob"], rel=1e-10)
        assert list(a["psihat"]) == list(b["psihat"]) and a["rss"] == b["rss"]
        np.testing.assert_allclose(b["EN"], a["EN"], rtol=1e-9, atol=1e-11)


# ---- the batches of the GPU file, from the oracle alone

def exist_probs(S, seqs, quals):
    """exist_prob of every sequence read as one with the motif (final quality 0)"""
    x = perturbed(engine(S))
    qs = []
    for q in quals:
        q = q.copy()
        q[-1] = 0
        qs.append(q)
    order = sorted(range(len(seqs)), key=lambda k: -len(seqs[k]))
    got = oracle_map(oracle_with(S, x), lambda o, k: o.scan_seq(seqs[k], qs[k])["exist_prob"], order)
    out = np.zeros(len(seqs))
    out[order] = got
    return out


@pytest.mark.parametrize("name,S,make", la.ALL_BATCHES, ids=["%s-%d" % (n, S) for n, S, _ in la.ALL_BATCHES])
def test_the_motif_parses_in_the_batches_of_the_gpu_file(name, S, make):
    """at least three quarters of every batch's sequences have a parse with the motif; a batch of the motif-conditioned products
    has at least two sequences with exist_prob >= cond_check.E_MIN"""
    seqs, quals = make(S)
    if name in ("train", "many"):          # (relabelled: every sequence twice)
        seqs, quals = seqs[::2], quals[::2]
    e = exist_probs(S, seqs, quals)
    assert np.mean(e > 0.0) >= la.PARSE_SHARE, e
    if name == "product":
        assert np.sum(e >= cd.E_MIN) >= 2, e


@pytest.mark.parametrize("S", la.WEIGHTED)
def test_the_world_shifts_put_exist_prob_in_mid_range(S):
    """la.WORLD_SHIFT on la.product_batch(S), from the oracle alone: every sequence has e >= cond_check.E_MIN or no parse with the
    motif at all (reference 2 of tests/world_check.py holds for the whole batch), and at least one has 0.05 <= e <= 0.95.  For
    such a sequence the motif world's context reference differs from the mixture's by more than 0.01: the mixture returned in place
    of the world (Z(ari, nasi) for Z(ari), or the mixture's terminals as the seed of the outside sweep) cannot pass the GPU file's
    motif-world checks, which it does wherever e is about 1."""
    from tests import ctx_check as cc, world_check as wc
    from tests.test_cond_cpu import motif_heavy
    pattern = la.PATTERN[S]
    seqs, quals = la.product_batch(S)
    o, on = cc.ctx_oracle(pattern, 50, 30), cc.ctx_oracle(pattern, 50, 30)
    x = motif_heavy(perturbed(engine(S)), o.hmm(), by=la.WORLD_SHIFT[S])
    xn = cd.none_params(x, o.hmm())
    refs = [wc.table_worlds(o, on, x, xn, s, q, ("context",)) for s, q in zip(seqs, quals)]
    es = [r["e"] for r in refs]
    assert all(r["e"] >= cd.E_MIN or not np.isfinite(r["Zari"]) for r in refs), es
    mid = [r for r in refs if la.E_MID[0] <= r["e"] <= la.E_MID[1]]
    assert mid, es
    differ = [np.abs(r["motif"]["context"] - r["mixed"]["context"]).max() for r in mid]
    print("S %d, shift %g: e %s, |motif - mixed| of the mid-range sequences %s" % (S, la.WORLD_SHIFT[S], es, differ))
    assert max(differ) > 0.01, (es, differ)


# ---- the log-space rule headers of the posterior products above 64 states

PRODUCTS = ("context", "node", "joint", "stem", "access", "cond", "helix", "loop")
ACCESS_WIDTH = 16


@pytest.mark.parametrize("product", PRODUCTS)
@pytest.mark.parametrize("S", la.WEIGHTED)
def test_log_space_product_rules_match_the_tables(S, product):
    """The LOG form of every product's CPU driver -- the rule headers the fused scan kernel runs behind its sweeps, over dense
    tables -- on la.product_batch(S) against the table reference and with the assert_* function the GPU file uses for that
    product: a failure here is a rule that is wrong above 64 states, a failure of the GPU file alone is the kernel's mapping of
    states to lanes, chunks and scratch."""
    from tests import access_check as ac, ctx_check as cc, helix_check as hc, joint_check as jc, loop_check as lc, node_check as nc
    from tests import stem_check as sc
    pattern = la.PATTERN[S]
    seqs, quals = la.product_batch(S)
    eng = engine(S)
    # (helices and loops at the parameters of their own files, as the GPU file runs them)
    x = hc.helix_params(eng) if product == "helix" else lc.loop_params(eng) if product == "loop" else perturbed(eng)
    M = eng.n_node
    args = (pattern, "~T2004~", 50, 30, 1e-4, 0.1, 0)
    if product == "cond":
        o, on = cd.world_oracles(lambda: cc.ctx_oracle(pattern, 50, 30), x)
        drv = cd.CondDriver(*args)
    else:
        o = {"context": cc.ctx_oracle, "node": nc.node_oracle, "joint": jc.joint_oracle, "stem": sc.stem_oracle,
             "access": ac.access_oracle, "helix": hc.helix_oracle, "loop": lc.loop_oracle}[product](pattern, 50, 30)
        o.set_params(x)
    for k, (s, q) in enumerate(zip(seqs, quals)):
        L, what = len(s), (S, product, k)
        if product == "context":
            ref = cc.table_profile(o, s, q, x, bulge=L <= 97)
            got, used = cc.CtxDriver(*args).profile(x, s, q, cc.CtxDriver.LOG)
            full = not np.isnan(ref[:, 4]).any()
            cc.assert_profile(got, ref, what=what, cols=range(7) if full else (0, 1, 2, 3, 6))
            np.testing.assert_allclose(got.sum(axis=1), 1.0, rtol=0, atol=1e-10)
        elif product == "node":
            ref = nc.table_profile(o, s, q, x)
            got, used = nc.NodeDriver(*args, n_node=M).profile(x, s, q, nc.NodeDriver.LOG)
            nc.assert_profile(got, ref, what=what, cols=range(M))
            np.testing.assert_allclose(got.sum(axis=1), 1.0, rtol=0, atol=1e-10)
        elif product == "joint":
            ref = jc.table_joint(o, s, q, x)
            got, counts, used = jc.JointDriver(*args, n_node=M).joint(x, s, q, jc.JointDriver.LOG)
            jc.assert_joint(got, ref, what=what)
            np.testing.assert_allclose(got.sum(axis=(1, 2)), 1.0, rtol=0, atol=1e-10)
        elif product == "stem":
            drv = sc.StemDriver(*args)
            assert np.array_equal(drv.slots, eng.stem_slots())
            ref = sc.table_stems(o, s, q, x)
            got, counts, used = drv.stems(x, s, q, sc.StemDriver.LOG)
            sc.assert_stem(got, sc.by_slot(ref, drv.slots), what=what)
        elif product == "access":
            ref, _ = ac.table_access(o, s, q, x, ACCESS_WIDTH)
            got, _, used = ac.AccessDriver(*args).access(x, s, q, ACCESS_WIDTH, ac.AccessDriver.LOG)
            ac.assert_access(got, ref, what=what)
        elif product == "helix":
            ref = hc.table_helices(o, s, q, x, kmax=hc.KMAX)
            got, _, used = hc.HelixDriver(*args).helices(x, s, q, hc.HelixDriver.LOG, kmax=hc.KMAX)
            hc.assert_helix(got, ref, what=what)
            hc.assert_properties(got, 1e-10, what=what)
        elif product == "loop":
            ref = lc.table_loops(o, s, q, x)
            r = lc.LoopDriver(*args).loops(x, s, q, lc.LoopDriver.LOG)
            used = r["form"]
            lc.assert_loop(r["cols"], ref[0], what=what)
            lc.assert_two(r["two"], ref[1], what=what)
            lc.assert_loop(r["P"], ref[2], what=(what, "P"))
        else:
            ref = cd.table_worlds(o, on, s, q)
            rec, used = drv.record(x, s, q, ref["kept"], cd.CondDriver.LOG)
            cd.check_record(rec, ref, L, min(L, 50), what=what)
        assert ref is not None and used == 1, what
