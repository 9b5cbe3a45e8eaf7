"""The usefulness mask of the train sweeps without a GPU: the host entry elemdp_useful_mask_host, which
runs the rule functions of rnaelem_amd/csrc/plan_rules.h that the plan kernel runs, against

  * the oracle: the mask must hold every entry (cell, plane) of planes P, E, M, B, 1, L in which some state has a finite inside AND
    a finite outside value in the oracle's tables (plane 2 follows the factorised rule 2 and is smaller than the oracle's by
    design; the pair entries A are not in the oracle's tables) -- zero missing entries, no exemptions;
  * a plain NumPy restatement of the rules in this file: equal, bit for bit.

On these cases the mask is not only a superset: it EQUALS the oracle's set on the six planes, and the test holds it to that (a
mask that grows skips less than it could).  The terms of the rules that read the unpaired flags only matter under a structure
constraint (the oracle's fix_rss switch): two such cases, with flags that are not all ones, against the oracle's tables there.

The sizes of the mask and of the oracle's set are printed per plane (pytest -s)."""
import os

import numpy as np
import pytest

from oracle import pyoracle as po
from rnaelem_amd import api, synth
from tests.util import gpath

P1, P5 = "((.*.))", "(.....)"
BIT = api.USEFUL_BITS
PLANES = dict(P=0, E=1, M=2, B=3, S1=4, S2=5, L=6)       # plane index of the oracle's tables
CHECKED = ("P", "E", "M", "B", "S1", "L")
M_MIN, MAX_LOOP = 10, 30


def n_base_seq(L):
    s = synth.synth_codes(1, L, seed=99 + L)[0]
    s[L // 3] = 0
    s[L // 2] = 0
    return s


def cases():
    out = []
    for L in (37, 60, 200):
        out.append(("synth L%d" % L, synth.synth_codes(2, L)[1]))
    out.append(("poly-A L60", np.full(60, 1, dtype=np.uint8)))
    out.append(("N bases L90", n_base_seq(90)))
    for rid, s, _ in po.read_fastq(gpath("tiny.fq")):
        out.append(("tiny.fq %s" % rid, np.asarray(s, dtype=np.uint8)))
    return out


CASES = cases()


def numpy_mask(kept, C, m_min=M_MIN, loop_cap=MAX_LOOP, unp=None):
    """The rules of plan_rules.h (useful_inside_cell, useful_loop_operands, useful_outside_cell), restated.  kept[(L+1), (W+1)]
    -> uint8 [(W+1), (L+1)]; unp[L]: the positions a structure constraint leaves unpaired (None: all of them)."""
    L, W = kept.shape[0] - 1, kept.shape[1] - 1
    unp = [True] * (L + 1) if unp is None else [bool(v) for v in unp] + [False]
    pair = lambda i, d: 0 <= i and 0 <= d <= W and i + d <= L and bool(kept[i, d])
    dmin = [next((d for d in range(1, W + 1) if pair(i, d)), 0) for i in range(L + 1)]
    left = lambda i, d: 0 <= d <= W and i + d <= L and dmin[i] > 0 and d >= dmin[i]
    e_ok = lambda i, d: i > 0 and d + 2 <= W and pair(i - 1, d + 2)
    m_ok = lambda i, d: 0 < i and i + d < L and d <= W and m_min <= d
    ins = {k: np.zeros((W + 1, L + 1), dtype=bool) for k in BIT}
    for d in range(0, min(W, L) + 1):
        for i in range(0, L - d + 1):
            j, dm = i + d, dmin[i]
            ins["L"][d, i] = True
            ins["P"][d, i] = pair(i, d)
            ins["E"][d, i] = e_ok(i, d)
            iA = False
            if 0 < dm < d:
                iA = dm < d - 1 and unp[j - 1] and ins["A"][d - 1, i]
                iA = iA or any(pair(j - sp, sp) and ins["S1"][d - sp, i] for sp in range(1, d - dm + 1))
            lok = left(i, d)
            iB = lok and iA
            i2 = lok and (pair(i, d) or (d > 0 and left(i, d - 1) and unp[j - 1] and ins["S2"][d - 1, i]))
            iM = m_ok(i, d) and (iB or (m_ok(i + 1, d - 1) and unp[i] and ins["M"][d - 1, i + 1]))
            ins["A"][d, i], ins["B"][d, i], ins["S2"][d, i], ins["S1"][d, i], ins["M"][d, i] = iA, iB, i2, i2 or iB, iM
    lm = np.zeros((W + 1, L + 1), dtype=bool)
    for d in range(0, min(W, L) + 1):
        for i in range(0, L - d + 1):
            if not e_ok(i, d):
                continue
            j = i + d
            for l in range(j, i + 1, -1):
                kmax = min(l - 2, i + C, i + loop_cap - (j - l))
                for k in range(i, kmax + 1):
                    if (k, l) != (i, j) and pair(k, l - k):
                        lm[k - i, i] = True
                        lm[j - l, l] = True
    u = {k: np.zeros((W + 1, L + 1), dtype=bool) for k in BIT}
    for d in range(min(W, L), -1, -1):
        for i in range(0, L - d + 1):
            j = i + d
            lok, mok, eok = left(i, d), m_ok(i, d), e_ok(i, d)
            uM = ins["M"][d, i] and (eok or (mok and m_ok(i - 1, d + 1) and unp[i - 1] and u["M"][d + 1, i - 1]))
            u1 = ins["S1"][d, i] and lok and any(pair(j, sp) and u["A"][d + sp, i] for sp in range(1, min(W - d, L - j) + 1))
            uB = ins["B"][d, i] and (uM or u1)
            step = d + 1 <= W and j < L
            uA = ins["A"][d, i] and (uB or (step and unp[j] and u["A"][d + 1, i]))
            u2 = ins["S2"][d, i] and (u1 or (lok and left(i, d + 1) and unp[j] and u["S2"][d + 1, i]))
            uL = eok or lm[d, i] or (step and u["L"][d + 1, i])
            u["P"][d, i], u["E"][d, i] = ins["P"][d, i], ins["E"][d, i]
            u["M"][d, i], u["B"][d, i], u["A"][d, i], u["S1"][d, i], u["S2"][d, i], u["L"][d, i] = uM, uB, uA, u1, u2, uL
    out = np.zeros((W + 1, L + 1), dtype=np.uint8)
    for k, b in BIT.items():
        out |= (u[k].astype(np.uint8) * b).astype(np.uint8)
    return out


def oracle_sets(pattern, C, seq):
    """kept pairs and, per plane, the [(W+1), (L+1)] boolean set {some state has a finite inside and a finite outside value}"""
    o = po.make_oracle(pattern, 50, C, min_bpp=1e-4, tau=0.1, lam=(1.0, 1.0))
    qual = np.full(len(seq) + 1, 10, dtype=np.uint8)
    qual[-1] = 0
    _, kept, _, _ = o.bpp(seq)
    r = o.train_seq(seq, qual, tables=True)
    both = np.isfinite(r["inside"]) & np.isfinite(r["outside"])          # [i][d][plane][state]
    return kept, {k: both[:, :, e, :].any(axis=2).T for k, e in PLANES.items()}


@pytest.mark.parametrize("C", [30, 5])
@pytest.mark.parametrize("pattern", [P1, P5])
def test_mask_holds_the_oracles_useful_entries(pattern, C, capsys):
    lines = []
    for name, seq in CASES:
        kept, sets = oracle_sets(pattern, C, seq)
        mask = api.useful_mask_host(kept, max_iloop=C)
        L, W = kept.shape[0] - 1, kept.shape[1] - 1
        assert mask.shape == (W + 1, L + 1)
        assert np.array_equal(mask, numpy_mask(kept, C)), "%s: host entry differs from the NumPy restatement" % name
        # (cells outside the band triangle i + d <= L carry no bits)
        dd, ii = np.meshgrid(np.arange(W + 1), np.arange(L + 1), indexing="ij")
        assert not mask[ii + dd > L].any(), name
        sizes = []
        for k in CHECKED:
            have = (mask & BIT[k]) != 0
            missing = sets[k] & ~have
            assert not missing.any(), "%s %s C %d: plane %s misses %d entries, first (d, i) = %s" % (
                name, pattern, C, k, int(missing.sum()), tuple(np.argwhere(missing)[0]))
            extra = have & ~sets[k]
            assert not extra.any(), "%s %s C %d: plane %s holds %d entries the oracle's set does not, first (d, i) = %s" % (
                name, pattern, C, k, int(extra.sum()), tuple(np.argwhere(extra)[0]))
            sizes.append("%s %d/%d" % (k, int(have.sum()), int(sets[k].sum())))
        k = "S2"
        sizes.append("S2 %d/(%d) A %d" % (int(((mask & BIT[k]) != 0).sum()), int(sets[k].sum()), int(((mask & BIT["A"]) != 0).sum())))
        n_cells = int((ii + dd <= L).sum())
        lines.append("%-12s %s C %2d cells %5d dead %5d | mask/oracle: %s" % (name, pattern, C, n_cells, int((mask[ii + dd <= L] == 0).sum()),
                                                                          "  ".join(sizes)))
    with capsys.disabled():
        print()
        print("\n".join(lines))


# Structure constraints: a multiloop of two and one of three branches with unpaired bases before, between and behind the branches
# (the steps of M, of the pair entries A and of plane 2 over unpaired positions: unp[i], unp[j - 1], unp[i - 1], unp[j]), beside a
# stem-loop in the exterior chain; the sequences pair G with C along the structure, so that the fixed structure has a finite energy.
FIX_CASES = [
    ("two branches L60", "..((..((....))...((.....))..))...(((....)))..".ljust(60, ".")),
    ("three branches L90", ".((.((.....))..(((....)))....((.....))...))....((..((.....))..))..".ljust(90, ".")),
]


def fix_inputs(db, W):
    """kept[(L+1), (W+1)] and unp[L] of a dot-bracket string, as load_batch derives them"""
    L = len(db)
    kept, stack = np.zeros((L + 1, W + 1), dtype=np.uint8), []
    for p, ch in enumerate(db):
        if ch == "(":
            stack.append(p)
        elif ch == ")":
            o = stack.pop()
            kept[o, p + 1 - o] = 1
    return kept, np.array([c == "." for c in db], dtype=np.uint8)


@pytest.mark.parametrize("C", [30, 5])
@pytest.mark.parametrize("pattern", [P1, P5])
def test_mask_under_a_structure_constraint(pattern, C, capsys):
    """the unp terms of the rules: host entry with non-trivial unpaired flags == the NumPy restatement, holds every entry of the
    oracle's fix_rss tables on P, E, M, B, 1, L, and differs from the mask without the flags (so the terms are in play)"""
    lines = []
    for name, db in FIX_CASES:
        L = len(db)
        W = min(L, 50)
        seq = np.array([{"(": 3, ")": 2, ".": 1}[c] for c in db], dtype=np.uint8)
        qual = np.full(L + 1, 10, dtype=np.uint8)
        qual[-1] = 0
        o = po.make_oracle(pattern, 50, C, min_bpp=1e-4, tau=0.1, lam=(1.0, 1.0), flags=po.DBG_FIX_RSS)
        r = o.train_seq(seq, qual, fix_rss=db, tables=True)
        assert np.isfinite(r["Zo"]), name                     # (the structure parses: the sets below are not empty)
        both = np.isfinite(r["inside"]) & np.isfinite(r["outside"])
        kept, unp = fix_inputs(db, W)
        assert not unp.all() and unp.any()
        mask = api.useful_mask_host(kept, max_iloop=C, unp=unp)
        assert np.array_equal(mask, numpy_mask(kept, C, unp=unp)), "%s: host entry differs from the NumPy restatement" % name
        assert not np.array_equal(mask, api.useful_mask_host(kept, max_iloop=C)), name
        sizes = []
        for k in CHECKED:
            have, want = (mask & BIT[k]) != 0, both[:, :, PLANES[k], :].any(axis=2).T
            assert want.any(), (name, k)
            missing = want & ~have
            assert not missing.any(), "%s %s C %d: plane %s misses %d entries, first (d, i) = %s" % (
                name, pattern, C, k, int(missing.sum()), tuple(np.argwhere(missing)[0]))
            if k in ("P", "M", "B", "S1"):      # (E and L take no unpaired flag in the rules: supersets under a constraint)
                assert np.array_equal(have, want), "%s %s C %d: plane %s is not the oracle's set" % (name, pattern, C, k)
            sizes.append("%s %d/%d" % (k, int(have.sum()), int(want.sum())))
        lines.append("%-18s %s C %2d | mask/oracle: %s" % (name, pattern, C, "  ".join(sizes)))
    with capsys.disabled():
        print()
        print("\n".join(lines))


def test_no_kept_pair_leaves_only_the_loop_chain_of_nothing():
    """a sequence without a kept pair has no E cell, so no entry of any plane is useful"""
    kept = np.zeros((61, 51), dtype=np.uint8)
    mask = api.useful_mask_host(kept, max_iloop=30)
    assert not mask.any()


def test_host_entry_rejects_bad_arguments():
    lib = api.load_library()
    kept = np.zeros((11, 11), dtype=np.uint8)
    out = np.zeros((11, 11), dtype=np.uint8)
    assert lib.elemdp_useful_mask_host(api._u8(kept), None, 10, 11, 30, 0, api._u8(out)) < 0      # W > L
    assert lib.elemdp_useful_mask_host(None, None, 10, 10, 30, 0, api._u8(out)) < 0
