"""Patterns of 63 to 128 interval states through every kernel family, against the oracle.  The largest
automaton of the other files has S = 59, 60 active states with the shadow copy of (0,0): below one wave.  Above 64 the kernels
map states to lanes, parts, chunks and LDS slices by code nothing else runs.  No checker and no tolerance of its own: the train
cases go through train_check.check_train_path, the scan and pair cases through pair_check.check_pair_path(scan=True), every
posterior product through the check_* function of its own GPU file, on the patterns and batches of tests/large_automata.py
(tests/test_large_automata_cpu.py: their state counts, the host rules and the parse shares of the batches, without a GPU).

What the engine sweeps (Engine::flatten_automaton): the shadow state, and with it the merged train schedule (n_pass 1), for
S < 127 -- at most 127 active states; S = 127 and 128 sweep the plain automaton under the reference's two outside passes
(n_pass 2).  So no handle has more than 128 active states, the `S > 128` branches of the exterior-chain kernels are out of
reach, and the shadow lane of the outside chain (ps == shadow among 128 lanes) always exists: test_train asserts n_pass.

Exterior-chain kernels: group_geometry launches k4_in_ext and the outside chain with 512 threads (the four-fold blocked chain)
for every group of at most 1024 sequences, whatever the state count; 128 threads for a larger group, for the outside chain of
the deterministic mode, and under option dbg 8192 (the plain chain without the fetch ahead).  Every batch here is one small group,
so "default" runs both chains in the blocked form, "deterministic" the outside chain in the plain form and "plain-chain" (dbg
8192) both in the plain form: nparts = 128 / n_active = 1 from S = 64 (65 active states) in all of them, 2 at S = 63.  The LDS
ring of the chain's last rows (ext_ring_doubles: 64 rows at W = 50, at most 48 KiB) exists up to 96 active states -- S = 63 to 78
-- and not for S = 126, 127, 128, which read the chain from the global table.

Band kernels (the forms launch_lin_group names under ELEMDP_LDS_DEBUG): the table-driven programs need lists that fit them
(every pattern here but S = 127, with the pruned lists) and an automaton blob of at most 4096 ints, which is staged whole: S = 63,
64 and 65 run them (form fp2), S = 78 to 128 the general kernels that read the blob from global memory (form generic), with 127
states in one cell of a workgroup's 256 lanes at cpb = 2; option fast 0 at S = 64 gives the general kernels with the staged blob
(form staged); test_train asserts which.

Log-space pipeline (pipeline 3): wave_gather.h's second state chunk (lane c * 64 + lane, c = 1) from 65 active states.  The
option names two different pipelines.  Under train_eval it is the batch pipeline of train_kernels.hip (the "pipeline3" cases of
test_train).  Under a scan-family call it is the log-space form of that call: the fused per-sequence kernel k_dp<DP_SCAN> of
kernels.hip, one workgroup per sequence on dense tables, which also takes the sequences the range check of the scaled-linear
form hands over.  Its sweeps merge tuples in both state chunks, and its per-workgroup scratch is sized by the state count
(tmp: 3 (Lmax + 1) S doubles; jnt.vec: 5 S per thread; acc.vec: 2 S per lane of the first wave; hlx.vec: 2 S per thread).  The
tests named
*_in_the_log_space_form run it on the batches and against the references of the scaled-linear cases, and
test_both_forms_in_one_call lets the range check split one batch between the two forms."""
import numpy as np
import pytest

from rnaelem_amd import api
from tests import cond_check as cd
from tests import ctx_check as cc
from tests import helix_check as hc
from tests import large_automata as la
from tests import loop_check as lc
from tests import test_access_gpu as t_access
from tests import test_cond_gpu as t_cond
from tests import test_ctx_gpu as t_ctx
from tests import test_helix_gpu as t_helix
from tests import test_joint_gpu as t_joint
from tests import test_loop_gpu as t_loop
from tests import test_node_gpu as t_node
from tests import test_node_mea_gpu as t_mea
from tests import test_stem_gpu as t_stem
from tests import test_world_gpu as t_world
from tests import train_check as tc
from tests import world_check as wc
from tests.mea_mirror import pair_matrix
from tests.pair_check import check_pair_path, oracle_refs
from tests.sample_check import Driver, check_sample_path
from tests.test_cond_cpu import motif_heavy
from tests.test_pair_posterior_gpu import perturbed
from tests.test_pair_shapes_gpu import oracle_maker
from tests.test_train_shapes_gpu import LINE

pytestmark = pytest.mark.gpu

PAR = "~T2004~"
W, C = 50, 30
TABLE_DRIVEN = {"fp2-waves", "fp2", "fast"}
BLOB_STAGED_WHOLE = 4096        # ints: Engine::prepare_lin stages the whole automaton blob up to this size, else its small part


def engine(S, opts=()):
    eng = api.Engine(la.PATTERN[S], PAR, W, C, 1e-4, 0.1, 0, 0)
    for k, v in opts:
        eng.set_option(k, v)
    return eng


_X = {}


def params(S):
    if S not in _X:
        _X[S] = perturbed(engine(S))
    return _X[S]


def loaded(S, seqs, quals, opts=()):
    eng = engine(S, opts)
    eng.load_batch(seqs, quals)
    return eng, params(S)


@pytest.fixture
def forms(monkeypatch, capfd):
    """sets ELEMDP_LDS_DEBUG; forms() returns (k4_in, k4_out, stage_ext, ext_nt, ext_ring, n_pass, combine) of every
    launch_lin_group since the last call"""
    monkeypatch.setenv("ELEMDP_LDS_DEBUG", "1")
    return lambda: [m.groups()[1:] for m in map(LINE.search, capfd.readouterr().err.splitlines()) if m]


# ---- refusals

@pytest.mark.parametrize("S,pattern", la.REFUSED, ids=[str(S) for S, _ in la.REFUSED])
def test_patterns_above_128_states_are_refused(S, pattern):
    with pytest.raises(api.ElemdpError, match="more than 128 interval states") as e:
        api.Engine(pattern, PAR, W, C, 1e-4, 0.1, 0, 0)
    assert e.value.code == -1


def test_a_pattern_of_128_states_constructs():
    eng = engine(128)
    assert eng.describe()["S"] == 128 and eng.describe()["layout"]["S"] == 128


# ---- train

TRAIN_OPTS = {
    "default": (),
    "deterministic": (("deterministic", 1),),
    "plain-chain": (("dbg", 8192),),
    "fast0": (("fast", 0),),
    "pipeline3": (("pipeline", 3),),
}
TRAIN_CASES = [(S, name) for S in la.ACCEPTED for name in ("default", "deterministic")] + \
              [(S, "plain-chain") for S in (64, 78, 126, 128)] + [(64, "fast0")] + [(S, "pipeline3") for S in la.LOG_SPACE]
_TRAIN_REFS = {}


def train_refs(S, name, make):
    """the oracle's rows of a batch, computed once for all its option sets"""
    if (S, name) not in _TRAIN_REFS:
        seqs, quals = make(S)
        _TRAIN_REFS[(S, name)] = seqs, quals, tc.oracle_train_refs(oracle_maker(la.PATTERN[S], W, C, params(S)), seqs, quals)
    return _TRAIN_REFS[(S, name)]


def assert_motif_parses(refs, quals):
    """three quarters of the batch's sequences, under either label, are not skipped by the oracle"""
    n = len(quals) // 2
    got = refs.unskipped(quals)
    assert got[0] >= la.PARSE_SHARE * n and got[1] >= la.PARSE_SHARE * n, got


def check_forms(S, name, seen, lay):
    """lay: describe()["layout"] of the engine, the automaton a train evaluation sweeps"""
    if name == "pipeline3":
        assert not seen
        return
    shadow = S < la.SHADOW_BELOW
    assert seen, "no launch_lin_group line"
    band = {"generic"} if lay["n_ints"] > BLOB_STAGED_WHOLE else TABLE_DRIVEN if lay["fp_ok"] and name != "fast0" else {"staged"}
    assert (band == {"generic"}) == (S > 65)
    for k4_in, k4_out, stage_ext, ext_nt, ext_ring, n_pass, combine in seen:
        assert {k4_in, k4_out} <= band, (k4_in, k4_out, band)
        assert (stage_ext, ext_ring) == ("1", "1")
        assert ext_nt == ("128" if name == "plain-chain" else "512"), ext_nt
        assert n_pass == ("1" if shadow else "2"), n_pass
        assert combine == ("1" if shadow or name == "deterministic" else "0"), combine


@pytest.mark.parametrize("S,name", TRAIN_CASES, ids=["%d-%s" % c for c in TRAIN_CASES])
def test_train(S, name, forms):
    """Twelve rows (six sequences of L 40 .. 131 under both labels): seq_stats, the count columns, fn, gr and the partial vector
    against the oracle, a repeated evaluation.  Which chain form each option set runs, and where nparts is 1 and the ring is
    gone: the module's docstring; check_forms asserts what the launcher reports (ext_nt of the inside chain, n_pass, the band
    form)."""
    seqs, quals, refs = train_refs(S, "train", la.train_batch)
    assert_motif_parses(refs, quals)
    eng, x = loaded(S, seqs, quals, TRAIN_OPTS[name])
    _, res, stats, counts = tc.check_train_path(eng, seqs, quals, x, oracle_maker(la.PATTERN[S], W, C, x), refs=refs)
    check_forms(S, name, forms(), eng.describe()["layout"])
    if name == "deterministic":         # bit for bit from one evaluation to the next
        res2 = eng.train_eval(x)
        c2 = eng.seq_counts()
        assert res2[0] == res[0] and np.array_equal(res2[1], res[1])
        assert np.array_equal(eng.seq_stats(), stats, equal_nan=True)
        assert all(np.array_equal(c2[key], counts[key]) for key in tc.COUNTS)


@pytest.mark.parametrize("S", la.LOG_SPACE)
def test_train_on_seventy_short_sequences(S, forms):
    """One group of 70 sequences (L 52 .. 76 under both labels): 70 workgroups per chain launch and per band diagonal, still
    the blocked chain (a group leaves it above 1024 sequences only: test_one_group_too_large_for_the_exterior_ring of
    test_train_shapes_gpu.py)."""
    seqs, quals, refs = train_refs(S, "many", la.many_batch)
    assert_motif_parses(refs, quals)
    eng, x = loaded(S, seqs, quals)
    tc.check_train_path(eng, seqs, quals, x, oracle_maker(la.PATTERN[S], W, C, x), refs=refs)
    check_forms(S, "default", forms(), eng.describe()["layout"])


# ---- scan and pairs

GAMMAS = (0.5, 1.0, 4.0)


PIPELINE3 = (("pipeline", 3),)
_REFS = {}


def cached(key, compute):
    """the oracle's references of a batch at params(S), computed once for every option set that runs it (as _TRAIN_REFS)"""
    if key not in _REFS:
        _REFS[key] = compute()
    return _REFS[key]


def pair_run(S, seqs, quals, opts=(), refs=None):
    eng, x = loaded(S, seqs, quals, opts)
    refs, res, mea = check_pair_path(eng, seqs, quals, x, oracle_maker(la.PATTERN[S], W, C, x), gammas=GAMMAS, scan=True, refs=refs)
    e = [r["scan"]["exist_prob"] for r in refs]
    if ("pipeline", 3) in opts:          # (no sum pass on the batch, so no sequence handed on by the range check)
        assert eng.last_timing()[2] == 0
    return refs, res, mea, e


def scan_refs(S):
    seqs, quals = la.scan_batch(S)
    return seqs, quals, cached((S, "scan"), lambda: oracle_refs(oracle_maker(la.PATTERN[S], W, C, params(S)), seqs, quals))


@pytest.mark.parametrize("S", la.SCAN)
def test_scan_and_pairs(S):
    """pair list, P and unpaired against the oracle, MEA against the mirror and the optimum, scan records (start, end, inner,
    exist_prob, Ys, Ye, rss, psihat, E[N]) against the oracle's; one sequence of the four is marked as without the motif"""
    seqs, quals, refs = scan_refs(S)
    refs, res, mea, e = pair_run(S, seqs, quals, refs=refs)
    assert sum(v > 0.0 for v in e) >= la.PARSE_SHARE * len(seqs), e
    assert sum(len(r[2]) for r in res) > 0


@pytest.mark.parametrize("S", la.LOG_SCAN)
def test_scan_and_pairs_in_the_log_space_form(S):
    """The batch of test_scan_and_pairs under pipeline 3: k_dp<DP_SCAN> runs the whole schedule of every sequence on dense tables
    -- both chunks of merge_tuples in its sweeps, the constrained second passes, sweep_cyk and the trace-back, PairLog -- on 65
    active states (S = 64), on a pattern whose blob the band kernels do not stage whole (78) and on the plain automaton of 128
    states.  The same references and checks as the scaled-linear form."""
    seqs, quals, refs = scan_refs(S)
    refs, res, mea, e = pair_run(S, seqs, quals, opts=PIPELINE3, refs=refs)
    assert sum(v > 0.0 for v in e) >= la.PARSE_SHARE * len(seqs), e
    assert sum(len(r[2]) for r in res) > 0


def test_scan_and_pairs_with_two_slots_reused():
    """S = 126, option group 2: five unsorted sequences in three groups on two slots"""
    seqs, quals = la.group2_batch(126)
    refs, res, mea, e = pair_run(126, seqs, quals, opts=(("group", 2),))
    assert sum(v > 0.0 for v in e) >= la.PARSE_SHARE * len(seqs), e


def test_scan_and_pairs_across_the_row_blocks():
    """S = 64, L = 257: the second 256-row block of k_pair_seq and k_pair_mea on an automaton of more than 64 active states"""
    seqs, quals = la.long_batch(64)
    refs, res, mea, e = pair_run(64, seqs, quals)
    assert all(v > 0.0 for v in e), e
    assert refs[0]["P"] is not None and len(res[0][3]) == 257 and len(res[0][2]) > 0


# ---- posterior products

@pytest.fixture(scope="module", params=la.WEIGHTED)
def product(request):
    """(S, seqs, quals, x, exist_prob per sequence from the oracle's scan)"""
    S = request.param
    seqs, quals = la.product_batch(S)
    x = params(S)
    refs = oracle_refs(oracle_maker(la.PATTERN[S], W, C, x), seqs, quals)
    e = [r["scan"]["exist_prob"] for r in refs]
    assert sum(v > 0.0 for v in e) >= la.PARSE_SHARE * len(seqs), e
    assert sum(v >= cd.E_MIN for v in e) >= 2, e
    return S, seqs, quals, x, refs


# Every product below runs twice on the same batch and against the same references (cached: the oracle is the slow part): in the
# scaled-linear form, and -- the tests named *_in_the_log_space_form, option pipeline 3 -- through k_dp<DP_SCAN> and the product's
# block behind its sweeps (CtxLog, NodeLog, JointLog, StemLog, AccLog, the two worlds of cond_p0 / cond_p1, the sample stacks),
# with the per-lane scratch sized by the state count.  The log-space runs take the tolerances the product
# files give that form in their lambda = 40 tests, and assert that no sequence was handed on by a range check: nothing ran the
# sum passes.

def product_engine(product, log):
    S, seqs, quals, x, _ = product
    eng, _ = loaded(S, seqs, quals, PIPELINE3 if log else ())
    return eng


def assert_log_form(eng, log):
    if log:
        assert eng.last_timing()[2] == 0


def context(product, log):
    S, seqs, quals, x, _ = product
    eng = product_engine(product, log)

    def make():
        o = cc.ctx_oracle(la.PATTERN[S], W, C)
        o.set_params(x)
        return o
    refs = cached((S, "ctx"), lambda: t_ctx.table_refs(make, seqs, quals, x))
    assert all(r is not None for r in refs)
    if log:
        t_ctx.check_profiles(eng, x, seqs, refs, what=(S, "log"), row_atol=1e-10)
    else:
        t_ctx.check_profiles(eng, x, seqs, refs, what=S)
    assert_log_form(eng, log)


def test_context_profiles(product):
    context(product, False)


def test_context_profiles_in_the_log_space_form(product):
    context(product, True)


def node_refs(S, seqs, quals, x):
    return cached((S, "node"), lambda: t_node.table_refs(t_node.oracle_with(la.PATTERN[S], x, W, C), seqs, quals, x))


def node(product, log):
    S, seqs, quals, x, _ = product
    eng = product_engine(product, log)
    make = t_node.oracle_with(la.PATTERN[S], x, W, C)
    refs = node_refs(S, seqs, quals, x)
    assert all(r is not None for r in refs)
    if log:
        t_node.check_profiles(eng, x, seqs, quals, refs, make=make, what=(S, "log"), row_atol=1e-10)
    else:
        t_node.check_profiles(eng, x, seqs, quals, refs, make=make, what=S)
    assert_log_form(eng, log)


def test_node_profiles(product):
    node(product, False)


def test_node_profiles_in_the_log_space_form(product):
    node(product, True)


def joint(product, log):
    S, seqs, quals, x, _ = product
    eng = product_engine(product, log)
    refs = cached((S, "joint"), lambda: t_joint.table_refs(t_joint.oracle_with(la.PATTERN[S], x, W, C), seqs, quals, x))
    assert all(r is not None for r in refs)
    if log:
        t_joint.check_joint(eng, x, seqs, refs, what=(S, "log"), row_atol=1e-10)
    else:
        t_joint.check_joint(eng, x, seqs, refs, what=S)
    assert_log_form(eng, log)


def test_joint_profiles(product):
    joint(product, False)


def test_joint_profiles_in_the_log_space_form(product):
    joint(product, True)


def stems(product, log):
    S, seqs, quals, x, _ = product
    eng = product_engine(product, log)
    make = t_stem.oracle_with(la.PATTERN[S], x, W, C)
    refs = cached((S, "stem"), lambda: t_stem.table_refs(make, seqs, quals, x))
    assert all(r is not None for r in refs)
    counts, _, _ = t_stem.check_stems(eng, x, seqs, refs, what=(S, "log") if log else S)
    assert_log_form(eng, log)
    t_stem.check_en(make, seqs, quals, refs, counts, eng.stem_slots(), what=S)


def test_stem_profiles(product):
    stems(product, False)


def test_stem_profiles_in_the_log_space_form(product):
    stems(product, True)


def access(product, width, log):
    S, seqs, quals, x, _ = product
    eng = product_engine(product, log)
    refs = cached((S, "access", width),
                  lambda: t_access.table_refs(t_access.maker(la.PATTERN[S], x, W, C), seqs, quals, x, width))
    assert all(r is not None for r in refs)
    if log:
        t_access.check_access(eng, x, seqs, refs, width, what=(S, width, "log"), atol=1e-10, unp_atol=1e-10)
    else:
        t_access.check_access(eng, x, seqs, refs, width, what=(S, width))
    assert_log_form(eng, log)


@pytest.mark.parametrize("width", [16, 64])
def test_accessibility(product, width):
    access(product, width, False)


@pytest.mark.parametrize("width", [16, 64])
def test_accessibility_in_the_log_space_form(product, width):
    access(product, width, True)


def conditional(product, log):
    S, seqs, quals, x, _ = product
    eng = product_engine(product, log)
    refs = cached((S, "cond"), lambda: t_cond.table_refs(t_cond.pattern_oracles(la.PATTERN[S], x, W, C), seqs, quals))
    assert sum(r["e"] >= cd.E_MIN for r in refs) >= 2, [r["e"] for r in refs]
    t_cond.check_batch(eng, x, seqs, refs, what=(S, "log") if log else S)
    assert_log_form(eng, log)


def test_conditional_pairs(product):
    conditional(product, False)


def test_conditional_pairs_in_the_log_space_form(product):
    conditional(product, True)


def node_mea(product, log):
    S, seqs, quals, x, _ = product
    eng = product_engine(product, log)
    refs = node_refs(S, seqs, quals, x)
    found = 0
    for K, gamma in ((1, 1.0), (4, 4.0)):
        found += sum(len(g["start"]) for g in t_mea.check_batch(eng, x, refs, gamma, K, what=(S, "log") if log else S))
    assert found > 0
    assert_log_form(eng, log)


def test_node_mea(product):
    node_mea(product, False)


def test_node_mea_in_the_log_space_form(product):
    node_mea(product, True)


def test_sampler(product):
    """70 samples per sequence (a full lane round of k_sample and a partial one): status, validity on the kept cells, the draws
    of the CPU driver, exact log-probabilities against the oracle.  Not the frequencies against the posteriors (check_sample_path
    without refs): their bound, five standard deviations + 2e-3, is meant for thousands of samples -- at 70 a single draw of one
    of the many cells below 1e-3 is outside it."""
    S, seqs, quals, x, _ = product
    eng, _ = loaded(S, seqs, quals)
    drv = Driver(la.PATTERN[S], PAR, W, C)
    drv.set_fast(True)
    out = check_sample_path(eng, seqs, quals, x, oracle_maker(la.PATTERN[S], W, C, x), 70, seed=S, drv=drv, n_check=6,
                            what="S %d" % S)
    assert all(st == eng.SAMPLED for _, _, _, st in out["res"])
    assert out["total"] >= 70          # (the driver drew at least one sequence's samples in the scaled-linear form)


def test_sampler_in_the_log_space_form(product):
    """pipeline 3: every sequence is sampled by k_dp<DP_SCAN> on its dense inside tables, walking the sample stacks of the
    state-count-sized scratch; that form has no CPU driver (section E of test_sample_shapes_gpu.py), so: status, validity on the
    kept cells, and the exact log-probability of six drawn derivations per sequence against Oracle.derivation_logz.  70 samples
    and no frequency check, for the reason test_sampler gives."""
    S, seqs, quals, x, _ = product
    eng = product_engine(product, True)
    out = check_sample_path(eng, seqs, quals, x, oracle_maker(la.PATTERN[S], W, C, x), 70, seed=S, n_check=6, log_all=True,
                            what="S %d pipeline 3" % S)
    assert all(st == eng.SAMPLED for _, _, _, st in out["res"])
    assert eng.last_timing()[2] == 0


# ---- helices and loops (DESIGN.md sections 23 and 24)
#
# Their own files stop at S = 65, one state on the second pass of the strided state loops (`for (s = lane; s < S; s += 64)` of
# k_loop_items, the HelixWave policy of k_helix_chains).  Here: a full second pass (S = 126 with the shadow state, 128 without it
# and under n_pass 2), the general band kernels and the chains without the LDS ring under them, and in the log-space form the
# S-sized per-thread vectors of HelixLog and LoopLog.  At the parameters of their own files (helix_check.helix_params,
# loop_check.loop_params) and against the table references: the CPU drivers take a quarter of a minute per sequence here, and
# tests/test_large_automata_cpu.py holds their LOG form to these same references.

def helix_case(S, seqs, quals):
    x = hc.helix_params(engine(S))
    make = t_helix.oracle_with(la.PATTERN[S], x, W, C)
    return x, cached((S, "helix"), lambda: t_helix.table_refs(make, seqs, quals, x, kmax=t_helix.KMAX))


def loop_case(S, seqs, quals):
    x = lc.loop_params(engine(S))
    return x, cached((S, "loop"), lambda: t_loop.table_refs(t_loop.oracle_with(la.PATTERN[S], x, W, C), seqs, quals, x))


def helices(S, seqs, quals, log, opts=()):
    x, refs = helix_case(S, seqs, quals)
    assert all(r is not None for r in refs)
    eng, _ = loaded(S, seqs, quals, (PIPELINE3 if log else ()) + opts)
    _, dense = t_helix.check_helices(eng, x, seqs, refs, kmax=t_helix.KMAX, what=(S, "log", opts) if log else S, log=log)
    assert_log_form(eng, log)
    if S == 128:
        assert max(g[:, :, 4:].max() for g in dense) > 0.05          # (the planted stems: helices of five pairs and more)
    return eng


def loops(S, seqs, quals, log, opts=()):
    x, refs = loop_case(S, seqs, quals)
    assert all(r is not None for r in refs)
    eng, _ = loaded(S, seqs, quals, (PIPELINE3 if log else ()) + opts)
    closing, _, _ = t_loop.check_loops(eng, x, seqs, refs, what=(S, "log", opts) if log else S, log=log)
    assert_log_form(eng, log)
    assert sum(len(c[2]) for c in closing) > 0
    return eng


def test_helix_posteriors(product):
    helices(*product[:3], False)


def test_helix_posteriors_in_the_log_space_form(product):
    helices(*product[:3], True)


def test_loop_posteriors(product):
    loops(*product[:3], False)


def test_loop_posteriors_in_the_log_space_form(product):
    loops(*product[:3], True)


@pytest.mark.parametrize("run", [helices, loops], ids=["helix", "loop"])
def test_a_workgroup_of_the_log_space_form_takes_two_sequences_of_128_states(run):
    """pipeline 3 with option slots 2 on the three planted sequences of S = 128: one workgroup takes two sequences on the same
    S-sized scratch (d_hx_vec_: 2 S doubles per thread at (blockIdx.x kThreads + tid) 2 S, addressed by the workgroup and not by
    the sequence); the references of the cases above"""
    seqs, quals = la.product_batch(128)
    eng = run(128, seqs, quals, True, opts=(("slots", 2),))
    assert (eng.slot_status()["slots"], eng.n_seq) == (2, 3)


# ---- one world

def world_case(S, seqs, quals):
    """(x: params(S) with the pattern rows shifted by la.WORLD_SHIFT[S], table references of both worlds, all eight products)"""
    x = motif_heavy(params(S), cc.ctx_oracle(la.PATTERN[S], W, C).hmm(), by=la.WORLD_SHIFT[S])
    return x, cached((S, "world"), lambda: t_world.table_refs(la.PATTERN[S], W, x, seqs, quals))


def worlds(product, log):
    """Option world on more than 64 states: the launchers' move of zs to zs[4g + world], the outside sweep seeded with one
    world's terminals and k_world_empty under the general band kernels, the chains without the LDS ring and a handle without the
    shadow state; in the log-space form the two worlds of k_dp<DP_SCAN>.  Every sequence has e >= E_MIN and one lies in mid-range
    (tests/test_large_automata_cpu.py), so the world with the motif is neither the mixture nor the other world."""
    S, seqs, quals, _, _ = product
    x, refs = world_case(S, seqs, quals)
    es = [r["e"] for r in refs]
    assert all(r["e"] >= wc.E_MIN or not np.isfinite(r["Zari"]) for r in refs), es
    assert any(la.E_MID[0] <= e <= la.E_MID[1] for e in es), es
    eng, _ = loaded(S, seqs, quals, PIPELINE3 if log else ())
    got = t_world.check_worlds(eng, x, seqs, refs, what=(S, "log") if log else S)
    return eng, x, seqs, refs, got


def test_worlds(product):
    eng, x, seqs, refs, got = worlds(product, False)
    # a sequence whose world is empty is handed to the log-space form (k_world_empty): none here, in either world
    n_empty = {w: sum(not np.isfinite(r["Zari" if w == "motif" else "Znasi"]) for r in refs) for w in wc.WORLDS}
    assert n_empty == dict(motif=0, none=0)
    assert eng.last_timing()[2] == n_empty["none"]          # (of the last call of check_worlds: the world without the motif)
    eng.pair_posteriors(x, 0.0, world="motif")
    assert eng.last_timing()[2] == n_empty["motif"]
    # e X_motif + (1 - e) X_none = X_mixed on the engine's own outputs, at the oracle's e
    mixed = wc.engine_products(eng, x, "mixed", seqs)
    assert eng.world == "mixed"
    for k, r in enumerate(refs):
        wc.assert_mixture(mixed[k], got["motif"][k], got["none"][k], r["e"], what=(product[0], k, r["e"]))


def test_worlds_in_the_log_space_form(product):
    eng, _, _, _, _ = worlds(product, True)
    assert eng.last_timing()[2] == 0


# ---- both forms in one call

LAM = {64: 10.0, 128: 10.0}      # lambda of Engine.initial_params, chosen on the GPU: test_both_forms_in_one_call
MIXED_PRODUCTS = ("pairs", "context", "node", "access", "helix", "loop", "world")


@pytest.mark.parametrize("what", MIXED_PRODUCTS)
@pytest.mark.parametrize("S", la.MIXED_FORM)
def test_both_forms_in_one_call(S, what):
    """Option group 2, parameters Engine.initial_params(lambda) as in the lambda = 40 tests of the product files, planted
    sequences of L 40, 257, 70 and 131: the range check of the scaled-linear sum passes hands the sequences whose tables leave
    the double range to k_dp<DP_SCAN>, in chunks of two, and the others keep the planes of the scaled-linear form: both forms
    fill one call's output, the log-space form addressing it by launch position.  Pair posteriors (and MEA), context and node
    profiles and accessibility at width 16 against the oracle's references at these same parameters, with the tolerances of the
    log-space form; helix and loop posteriors against their table references likewise; "world": pairs and context in both worlds
    (the last call counted is context_profiles in the world with the motif).  lambda was chosen on an MI355X among 5, 10, 20,
    30, 40, 60, 80: at S = 64 and at S = 128 alike, in every one of the first four calls and in scan, lambda = 5 flags 1 sequence
    of the 4, lambda = 10 flags 3 (two chunks), and from lambda = 20 all 4 are flagged; so lambda = 10, flagged count 3, for
    both patterns."""
    seqs, quals = la.mixed_form_batch(S)
    eng = engine(S, (("group", 2),))
    eng.load_batch(seqs, quals)
    x = eng.initial_params(LAM[S])
    pattern = la.PATTERN[S]
    if what == "pairs":
        make = oracle_maker(pattern, W, C, x)
        check_pair_path(eng, seqs, quals, x, make, gammas=GAMMAS, refs=oracle_refs(make, seqs, quals))
    elif what == "context":
        def make():
            o = cc.ctx_oracle(pattern, W, C)
            o.set_params(x)
            return o
        t_ctx.check_profiles(eng, x, seqs, t_ctx.table_refs(make, seqs, quals, x), what=(S, "mixed"), row_atol=1e-10)
        eng.context_profiles(x)
    elif what == "node":
        make = t_node.oracle_with(pattern, x, W, C)
        t_node.check_profiles(eng, x, seqs, quals, t_node.table_refs(make, seqs, quals, x), what=(S, "mixed"), row_atol=1e-10)
    elif what == "access":
        refs = t_access.table_refs(t_access.maker(pattern, x, W, C), seqs, quals, x, 16)
        t_access.check_access(eng, x, seqs, refs, 16, what=(S, "mixed"), atol=1e-10, unp_atol=1e-10)
        eng.accessibility(x, 16)
    elif what == "helix":
        refs = t_helix.table_refs(t_helix.oracle_with(pattern, x, W, C), seqs, quals, x, kmax=t_helix.KMAX)
        t_helix.check_helices(eng, x, seqs, refs, kmax=t_helix.KMAX, what=(S, "mixed"), log=True)
        eng.helix_posteriors(x, 0.0, 1, t_helix.KMAX)
    elif what == "loop":
        refs = t_loop.table_refs(t_loop.oracle_with(pattern, x, W, C), seqs, quals, x)
        t_loop.check_loops(eng, x, seqs, refs, what=(S, "mixed"), log=True)
        eng.loop_posteriors(x, 0.0)
    else:
        # pairs and context in both worlds, with the checks and the tolerances of test_world_gpu's
        # test_sequences_out_of_the_double_range_take_the_log_space_form: the mixture identity at the conditional call's e, the
        # world without the motif against reference 1, P of both worlds against the conditional call
        prods = ("pairs", "context")
        refs = t_world.table_refs(pattern, W, x, seqs, quals, prods)
        got = {}
        for w in ("mixed",) + wc.WORLDS:
            got[w] = wc.engine_products(eng, x, w, seqs, prods)
            assert 1 <= eng.last_timing()[2] < len(seqs), (w, eng.last_timing()[2])
        con = eng.conditional_pairs(x, 0.0)
        for k in range(len(seqs)):
            L, Wk = len(seqs[k]), min(len(seqs[k]), W)
            wc.assert_mixture(got["mixed"][k], got["motif"][k], got["none"][k], con[k]["exist_prob"], what=(S, k), count_rtol=1e-12)
            for w in wc.WORLDS:
                np.testing.assert_allclose(got[w][k]["pairs"], pair_matrix(L, Wk, con[k]["i"], con[k]["j"], con[k]["p_" + w])[0],
                                           rtol=0, atol=1e-12, err_msg=str((S, w, k)))
            if np.isfinite(refs[k]["Znasi"]):
                wc.assert_world(got["none"][k], refs[k], "none", ("pairs", "unpaired", "context"), what=(S, k))
        eng.context_profiles(x, world="motif")
    n_flagged = int(eng.last_timing()[2])          # (of the product's own call, the last one)
    print("both forms, S %d, %s: lambda %g flags %d of %d" % (S, what, LAM[S], n_flagged, len(seqs)))
    assert 1 <= n_flagged < len(seqs), n_flagged
