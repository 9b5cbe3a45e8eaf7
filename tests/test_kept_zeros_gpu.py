"""A slot per sequence and the zeros it keeps (option own_slots) on the GPU.  With the option on, the second
train evaluation of a resident batch finds the exact zeros of the entries the usefulness mask calls useless still in its table
slots and stores none of them (Engine.slot_status()["zeros_kept"]); whatever may have written something else there -- another
batch, a scan-family call, debug_tables, a ranged evaluation, an option that changes the sweeps, the NaN poisoning -- makes the
next evaluation store them again.  Every result is held against a FRESH engine with own_slots 0, the path before the option,
evaluated at the same x: bit for bit in the deterministic mode (fn, gr, seq_stats, seq_counts), within the tolerances of
tests/test_live_blocks_gpu.py (tests/test_useful_mask_gpu.py::compare) in the default mode.
Every engine here turns the suite's NaN poisoning off (option poison 0): a poisoned evaluation never keeps zeros.  The batches are
small (14 to 20 sequences of L 24, 37, 60 and 90 in one batch); live_blocks 2 as well as 1, so that every diagonal is swept from
lists once."""
import numpy as np
import pytest

from rnaelem_amd import api, io
from tests.test_pair_posterior_gpu import perturbed
from tests.test_pair_shapes_gpu import batch
from tests.test_useful_mask_gpu import P1, P5, PAR, compare, has_dead_and_live_cells
from tests.util import gpath

pytestmark = pytest.mark.gpu

CONFIGS = [(P1, 50, 30), (P5, 20, 5), (P1, 20, 5), (P5, 50, 30)]      # pattern, W, C
LENS = [90, 37, 60, 37, 90, 60, 37, 60, 90, 37, 60, 90, 37, 60, 90, 37, 60, 90]


def make_batch(seed):
    """18 synthetic sequences of L 37, 60, 90 (some with N bases, both labels) and the two records of tests/golden/tiny.fq"""
    seqs, quals = batch(LENS, seed=seed)
    for _, s, q in io.read_fastq(gpath("tiny.fq")):
        seqs.insert(5, np.asarray(s, dtype=np.uint8))
        quals.insert(5, np.asarray(q, dtype=np.uint8))
    return seqs, quals


BATCHES = {"A": make_batch(11), "B": make_batch(12), "one": tuple(v[:1] for v in make_batch(11))}      # (B: the shape of A, other bases)


def engine(cfg, own, opts=()):
    pattern, W, C = cfg
    eng = api.Engine(pattern, PAR, W, C, 1e-4, 0.1, 0, 0)
    eng.set_option("poison", 0)
    eng.set_option("own_slots", own)
    for k, v in opts:
        eng.set_option(k, v)
    return eng


def points(eng):
    x0 = perturbed(eng)
    x1 = perturbed(eng, 0.3)
    x1[:-2] *= 0.5
    return x0, x1


def evaluate(eng, x):
    res = eng.train_eval(x)
    return res, eng.seq_stats(), {k: v.copy() for k, v in eng.seq_counts().items()}


_REF = {}


def reference(cfg, name, opts, which):
    """what a fresh engine with own_slots 0 and the options `opts` returns for batch `name` at point `which` (0 or 1): computed
    once per key, both points by the same engine, and never changed"""
    key = (cfg, name, tuple(opts))
    if key not in _REF:
        eng = engine(cfg, 0, opts)
        eng.load_batch(*BATCHES[name])
        for k, v in opts:      # (a load resets the range of the evaluation)
            if k.startswith("eval_"):
                eng.set_option(k, v)
        out = []
        for x in points(eng):
            out.append(evaluate(eng, x))
            assert not eng.slot_status()["zeros_kept"]
        _REF[key] = out
    return _REF[key][which]


def check(eng, cfg, name, opts, which, kept, what):
    """one evaluation at point `which`: the status, and the results against the reference with the same options"""
    det = bool(dict(opts).get("deterministic", 0))
    got = evaluate(eng, points(eng)[which])
    st = eng.slot_status()
    assert st["zeros_kept"] == kept, (what, st)
    compare(got, reference(cfg, name, opts, which), det, "%s %s, %s" % (cfg, opts, what))
    return st


@pytest.mark.parametrize("lb", [1, 2])
@pytest.mark.parametrize("cfg", CONFIGS)
def test_steady_state(cfg, lb):
    """x0, x1, x0: evaluations 2 and 3 keep the zeros, all three equal the reference, in the deterministic and the default mode"""
    eng = engine(cfg, 1, (("live_blocks", lb),))
    eng.load_batch(*BATCHES["A"])
    assert any(has_dead_and_live_cells(eng.useful_mask(k)) for k in range(eng.n_seq))
    for det in (1, 0):
        opts = (("live_blocks", lb), ("deterministic", det))
        eng.set_option("deterministic", det)
        for step, (which, kept) in enumerate(((0, False), (1, True), (0, True))):
            st = check(eng, cfg, "A", opts, which, kept, "evaluation %d" % (step + 1))
            assert st["slots"] == eng.n_seq
    ref = engine(cfg, 0)      # (the slots of the shared mapping: no more than the batch either)
    ref.load_batch(*BATCHES["A"])
    ref.train_eval(points(ref)[0])
    assert ref.slot_status() == {"zeros_kept": False, "slots": eng.n_seq}


def steady(eng, cfg, name, opts):
    check(eng, cfg, name, opts, 0, False, "first evaluation")
    check(eng, cfg, name, opts, 1, True, "second evaluation")


def base_opts(det, lb=1):
    return (("live_blocks", lb), ("deterministic", det))


@pytest.mark.parametrize("det", [1, 0])
@pytest.mark.parametrize("cfg", CONFIGS[:2])
def test_another_batch_of_the_same_shape(cfg, det):
    """the test with teeth: the live values of batch A lie where the dead entries of batch B are"""
    opts = base_opts(det)
    eng = engine(cfg, 1, opts)
    eng.load_batch(*BATCHES["A"])
    steady(eng, cfg, "A", opts)
    eng.load_batch(*BATCHES["B"])
    steady(eng, cfg, "B", opts)
    check(eng, cfg, "B", opts, 0, True, "third evaluation of B")
    eng.load_batch(*BATCHES["A"])
    steady(eng, cfg, "A", opts)


@pytest.mark.parametrize("call", ["scan", "pair_posteriors"])
@pytest.mark.parametrize("det", [1, 0])
def test_scan_family_call_between(det, call):
    cfg, opts = CONFIGS[0], base_opts(det, 2)
    eng = engine(cfg, 1, opts)
    eng.load_batch(*BATCHES["A"])
    steady(eng, cfg, "A", opts)
    getattr(eng, call)(points(eng)[1])
    steady(eng, cfg, "A", opts)


@pytest.mark.parametrize("det", [1, 0])
def test_debug_tables_between(det):
    """debug_tables (one resident sequence) repeats the evaluation with the generic kernels, which store every entry"""
    cfg, opts = CONFIGS[0], base_opts(det)
    eng = engine(cfg, 1, opts)
    eng.load_batch(*BATCHES["one"])
    assert has_dead_and_live_cells(eng.useful_mask(0))
    steady(eng, cfg, "one", opts)
    eng.debug_tables()
    steady(eng, cfg, "one", opts)


@pytest.mark.parametrize("det", [1, 0])
def test_ranged_evaluation_between(det):
    cfg, opts = CONFIGS[1], base_opts(det)
    eng = engine(cfg, 1, opts)
    eng.load_batch(*BATCHES["A"])
    steady(eng, cfg, "A", opts)
    ranged = opts + (("eval_first", 3), ("eval_count", 7))
    for k, v in ranged[2:]:
        eng.set_option(k, v)
    got = evaluate(eng, points(eng)[0])
    assert not eng.slot_status()["zeros_kept"]
    want = reference(cfg, "A", ranged, 0)
    # (the rows of the range; the rows outside it are what earlier evaluations of either engine left)
    assert got[0][2:] == want[0][2:]
    if det:
        assert got[0][0] == want[0][0] and np.array_equal(got[0][1], want[0][1]) and np.array_equal(got[1][3:10], want[1][3:10])
    else:
        assert got[0][0] == pytest.approx(want[0][0], rel=1e-10)
        np.testing.assert_allclose(got[0][1], want[0][1], rtol=1e-8, atol=1e-10)
        np.testing.assert_allclose(got[1][3:10], want[1][3:10], rtol=1e-10, atol=1e-10)
    eng.set_option("eval_first", 0)
    eng.set_option("eval_count", 0)
    steady(eng, cfg, "A", opts)


TOGGLES = {"useful_mask": (0, False), "live_blocks": (2, True), "loop_prepass": (0, True), "loop_outside": (0, True),
           "deterministic": (None, True)}      # option: (the other value, the state under it still keeps zeros)


@pytest.mark.parametrize("det", [1, 0])
@pytest.mark.parametrize("option", list(TOGGLES))
def test_option_toggled_between(option, det):
    cfg, opts = CONFIGS[0], base_opts(det)
    value, keeps = TOGGLES[option]
    if value is None:
        value = 1 - det
    eng = engine(cfg, 1, opts)
    eng.load_batch(*BATCHES["A"])
    steady(eng, cfg, "A", opts)
    other = tuple((k, v) for k, v in opts if k != option) + ((option, value),)
    eng.set_option(option, value)
    check(eng, cfg, "A", other, 0, False, "%s %s, first evaluation" % (option, value))
    check(eng, cfg, "A", other, 1, keeps, "%s %s, second evaluation" % (option, value))
    eng.set_option(option, dict(opts).get(option, 1))
    steady(eng, cfg, "A", opts)


@pytest.mark.parametrize("det", [1, 0])
def test_poisoned_evaluation_between(det):
    cfg, opts = CONFIGS[0], base_opts(det, 2)
    eng = engine(cfg, 1, opts)
    eng.load_batch(*BATCHES["A"])
    steady(eng, cfg, "A", opts)
    eng.set_option("poison", 1)
    for which in (0, 1):      # (every entry NaN before the sweeps: the zeros are stored, every time)
        check(eng, cfg, "A", opts, which, False, "poisoned evaluation %d" % (which + 1))
    eng.set_option("poison", 0)
    # (the poisoned evaluation stored every zero behind the NaN: what it left is a steady state)
    check(eng, cfg, "A", opts, 0, True, "behind the poisoned evaluations")


@pytest.mark.parametrize("det", [1, 0])
@pytest.mark.parametrize("option", ["slots", "group"])
def test_fallback_where_the_slots_are_fewer_than_the_batch(option, det):
    cfg, opts = CONFIGS[1], base_opts(det)
    eng = engine(cfg, 1, opts + ((option, 13),))
    eng.load_batch(*BATCHES["A"])
    for step, which in enumerate((0, 1, 0)):
        st = check(eng, cfg, "A", opts, which, False, "%s 13, evaluation %d" % (option, step + 1))
        # (option slots is the slot count of the calls that name no group; a train evaluation sizes its slots for its group)
        assert st["slots"] == (13 if option == "group" else eng.n_seq)
