"""Patterns of 63 to 130 interval states and the batches that tests/test_large_automata_cpu.py and
tests/test_large_automata_gpu.py share.

The CPU file checks, from the oracle alone, that every batch here lets the motif parse (PARSE_SHARE of its sequences) and that the
batches of the motif-conditioned products hold at least two sequences with exist_prob >= cond_check.E_MIN; the GPU file then runs
the same batches through the kernels.

Sequences: the deep-stem patterns have no parse on the synthetic sequences of synth.synth_batch, so every batch of the train and
scan cases holds planted hairpins G^h AAAA C^h (h at least the stem depth of every pattern of the table: 8) between short random
spacers, beside plain synthetic sequences."""
import numpy as np

from rnaelem_amd import synth
from tests import train_check as tc

# state count S (without the shadow copy of (0,0)), node count M, pattern
TABLE = [
    (63, 21, "(((.(...).(...).)))"),
    (64, 19, ".(.*.).(((.*.)))."),
    (65, 25, "(((((.*.))))).(((...)))"),
    (78, 29, "(((.*.)))(((.*.)))(((.*.)))"),
    (126, 29, ".*(.*.).(.*.).((((...))))*."),
    (127, 43, ".*(((((((.*.))))))).((((((((.*.))))))))*."),
    (128, 36, ".*(.*.).((.*.)).(((((((.*.)))))))."),
]
REFUSED = [
    (129, ".*((((((.*.)))))).*.(((((((.*.)))))))."),
    (130, ".*(.*.).(.*.).(((((...)))))*."),
]
PATTERN = {S: p for S, _, p in TABLE}
ACCEPTED = [S for S, _, _ in TABLE]
SHADOW_BELOW = 127       # Engine::flatten_automaton: the shadow copy of (0,0), and with it the merged train schedule, for S < 127
LOG_SPACE = (64, 127, 128)          # the patterns of the pipeline 3 and the many-sequence train cases
SCAN = (64, 65, 78, 126, 127, 128)  # the scan and pair cases (65: the other pattern above 64 states that runs table-driven)
LOG_SCAN = (64, 78, 128)            # the scan and pair cases in the log-space form (78: the first blob not staged whole)
WEIGHTED = (64, 126, 128)           # the patterns whose motif parses with weight: the posterior-product cases
MIXED_FORM = (64, 128)              # the cases with both forms of the scan family in one call
PARSE_SHARE = 0.75
STEM = 8                 # the deepest stem of the table (S = 127, 128)


def hairpin(h, loop=4):
    return [3] * h + [1] * loop + [2] * h


def planted(L, seed):
    """a sequence of exactly L >= 40 bases: hairpins G^h AAAA C^h of the depths below, in that order, at least one random base
    between two of them and behind the last, the other random bases dealt to the gaps; qualities 10, final quality 0.  The
    depths: a shallow hairpin in front for the patterns of three stems (S = 126, 128), two of STEM pairs from L = 52 for the
    patterns of two deep stems (S = 65, 127; no room for them at L = 40)"""
    rng = np.random.default_rng(seed)
    depths = (2, 2, STEM) if L < 52 else (2, STEM, STEM) if L < 110 else (3, STEM, STEM, STEM)
    n = len(depths)
    free = L - sum(2 * h + 4 for h in depths) - n
    assert free >= 0, (L, depths)
    gaps = np.bincount(rng.integers(0, n + 1, size=free), minlength=n + 1) + np.array([0] + [1] * n)
    s = []
    for k, h in enumerate(depths):
        s += [int(v) for v in rng.integers(1, 5, size=int(gaps[k]))] + hairpin(h)
    s += [int(v) for v in rng.integers(1, 5, size=int(gaps[n]))]
    assert len(s) == L
    q = np.full(L + 1, 10, dtype=np.uint8)
    q[-1] = 0
    return np.array(s, dtype=np.uint8), q


def random_seq(L, seed):
    (s,), (q,) = synth.synth_batch(1, L, seed=seed)
    return s, q


def mixed(lens, seed, planted_every=1):
    """one sequence per length: planted hairpins at every planted_every-th position of the list (0: nowhere), plain synthetic
    sequences at the others"""
    seqs, quals = [], []
    for k, L in enumerate(lens):
        s, q = planted(L, seed + 17 * k) if planted_every and k % planted_every == 0 else random_seq(L, seed + 17 * k)
        seqs.append(s)
        quals.append(q)
    return seqs, quals


# ---- train

TRAIN_LENS = (40, 57, 70, 97, 120, 131)
MANY_N = 35              # sequences of the many-sequence batch before relabelling (70 after)


def train_batch(S):
    """six sequences, L 40 .. 131, under both labels (12 rows)"""
    return tc.relabelled(*mixed(TRAIN_LENS, seed=1000 + S, planted_every=1 if S in (65, 78, 127, 128) else 2))


def many_batch(S):
    """70 short sequences (35 of L 52 .. 76 under both labels): one group of 70 workgroups per chain launch"""
    rng = np.random.default_rng(7000 + S)
    lens = [int(v) for v in rng.integers(52, 77, size=MANY_N)]
    return tc.relabelled(*mixed(lens, seed=7000 + S, planted_every=1 if S in (127, 128) else 2))


# ---- scan and pairs

SCAN_LENS = (40, 70, 97, 131)


def scan_batch(S):
    seqs, quals = mixed(SCAN_LENS, seed=2000 + S, planted_every=1 if S in (65, 78, 127, 128) else 2)
    quals[1][-1] = 5          # (one sequence marked as without the motif: its pairs are those of the parses without it)
    return seqs, quals


def group2_batch(S=126):
    """five sequences for option group 2: three groups reuse two slots"""
    return mixed((131, 40, 97, 70, 57), seed=2500 + S, planted_every=2)


def long_batch(S=64):
    """L = 257: the second 256-row block of the per-sequence kernels"""
    return mixed((257, 70), seed=2570 + S, planted_every=2)


def mixed_form_batch(S):
    """planted sequences of L 40 and 70 beside L 131 and 257 for the cases that run both forms of the scan family in one call:
    under parameters sharp enough the long ones leave the double range of the scaled-linear tables, the short ones do not"""
    return mixed((40, 257, 70, 131), seed=2600 + S)


# ---- posterior products (the motif-conditioned checks need exist_prob >= E_MIN)

PRODUCT_RANDOM = {64: ((70, 3064), (131, 3081)), 126: ((70, 3177), (131, 3143))}     # (L, seed of synth.synth_batch)


def product_batch(S):
    """64 and 126: plain synthetic sequences of L 70 and 131, both with exist_prob >= E_MIN (the seeds were chosen for that: at
    S = 126 most synthetic sequences of L 70 stay far below); 128: the planted 8-deep hairpin at L 40, 70, 131"""
    if S == 128:
        return mixed((40, 70, 131), seed=3000 + S)
    pairs = [random_seq(L, seed) for L, seed in PRODUCT_RANDOM[S]]
    return [s for s, _ in pairs], [q for _, q in pairs]


# ---- one world

# The shift of the pattern rows (test_cond_cpu.motif_heavy(x, hmm, by=shift) on perturbed(engine(S))) at which option world runs on
# product_batch(S): at the plain parameters every sequence of these batches has exist_prob between 0.997 and 1, and where e is about
# 1 the world with the motif is the mixture.  At these shifts every sequence keeps e >= cond_check.E_MIN (reference 2
# holds) and at least one has 0.05 <= e <= 0.95, so that the worlds and the mixture are three different things
# (tests/test_large_automata_cpu.py: test_the_world_shifts_put_exist_prob_in_mid_range).  e per sequence, from the oracle:
#   S = 64, shift -0.6: 0.114, 0.531;   S = 126, shift -0.3: 0.822, 1.000;   S = 128, shift -1.0: 0.030, 0.116, 0.933
WORLD_SHIFT = {64: -0.6, 126: -0.3, 128: -1.0}
E_MID = (0.05, 0.95)


ALL_BATCHES = (
    [("train", S, train_batch) for S in ACCEPTED] + [("many", S, many_batch) for S in LOG_SPACE] +
    [("scan", S, scan_batch) for S in SCAN] + [("group2", 126, group2_batch), ("long", 64, long_batch)] +
    [("product", S, product_batch) for S in WEIGHTED] + [("mixed", S, mixed_form_batch) for S in MIXED_FORM])
