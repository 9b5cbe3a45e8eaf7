"""The pair terms of the outside train sweep without a GPU: the host entry elemdp_pair_terms_host, which
runs the rule functions of rnaelem_amd/csrc/plan_rules.h (ha_rows, h1_stems) that the plan kernel runs, against

  * a brute-force NumPy restatement from the mask bytes: equal, word for word;
  * the transposition invariant: the triples (i, k, j) of `1(i,k) x stem (k,j) -> A(i,j)` read from ha_rows (by the stem cell) equal
    the ones read from h1_stems (by the left cell), and both are exactly the stems the inside pair phase walks for cells with
    UB_A whose operand 1(i,k) has UB_1;
  * the degenerate cases: no kept pair, the mask of all ones, W = 64 and W = 65.

The kept pairs come from the oracle's filter, the mask from elemdp_useful_mask_host.  The L = 200 cases print their counts
(pytest -s)."""
import functools

import numpy as np
import pytest

from oracle import pyoracle as po
from rnaelem_amd import api
from tests.test_useful_mask_cpu import CASES, P1, P5

UB_A, UB_1 = api.USEFUL_BITS["A"], api.USEFUL_BITS["S1"]


@functools.lru_cache(maxsize=None)
def kept_of(pattern, C, k):
    o = po.make_oracle(pattern, 50, C, min_bpp=1e-4, tau=0.1, lam=(1.0, 1.0))
    _, kept, _, _ = o.bpp(CASES[k][1])
    return np.ascontiguousarray(kept, dtype=np.uint8)


def dmin_of(kept):
    L, W = kept.shape[0] - 1, kept.shape[1] - 1
    return [next((d for d in range(1, W + 1) if i + d <= L and kept[i, d]), 0) for i in range(L + 1)]


def numpy_words(mask, kept):
    """ha_rows and h1_stems as the issue states them, cell by cell and bit by bit.  mask [(W+1), (L+1)], kept [(L+1), (W+1)]."""
    W, L = mask.shape[0] - 1, mask.shape[1] - 1
    dmin = dmin_of(kept)
    pair = lambda i, d: 0 <= i and 0 <= d <= W and i + d <= L and bool(kept[i, d])
    ha = np.zeros((W + 1, L + 1), dtype=np.uint64)
    h1 = np.zeros((W + 1, L + 1), dtype=np.uint64)
    for d in range(W + 1):
        for i in range(L - d + 1):
            j = i + d
            if pair(i, d):
                w = 0
                for b in range(1, W - d + 1):
                    ii = i - b
                    if ii >= 0 and dmin[ii] > 0 and b >= dmin[ii] and (mask[d + b, ii] & UB_A) and (mask[b, ii] & UB_1):
                        w |= 1 << (b - 1)
                ha[d, i] = w
            if dmin[i] > 0 and d >= dmin[i] and (mask[d, i] & UB_1):
                w = 0
                for sp in range(1, min(W - d, L - j) + 1):
                    if pair(j, sp) and (mask[d + sp, i] & UB_A):
                        w |= 1 << (sp - 1)
                h1[d, i] = w
    return ha, h1


def bits_of(word):
    word = int(word)
    return [b for b in range(64) if (word >> b) & 1]


def triples_ha(ha):
    """(i, k, j) of every bit: the stem cell (k, j - k) and its parent row i = k - b"""
    return {(k - (b + 1), k, k + d) for d, k in zip(*np.nonzero(ha)) for b in bits_of(ha[d, k])}


def triples_h1(h1):
    """(i, k, j) of every bit: the left cell (i, k - i) and the stem (k, k + sp)"""
    return {(i, i + d, i + d + b + 1) for d, i in zip(*np.nonzero(h1)) for b in bits_of(h1[d, i])}


def triples_inside(mask, kept):
    """the stems (k, j) the inside pair phase walks for the cells (i, j - i) with UB_A, whose operand 1(i, k) has UB_1"""
    W, L = mask.shape[0] - 1, mask.shape[1] - 1
    dmin = dmin_of(kept)
    out = set()
    for d in range(W + 1):
        for i in range(L - d + 1):
            if not (mask[d, i] & UB_A) or not 0 < dmin[i] < d:
                continue
            j = i + d
            for sp in range(1, d - dmin[i] + 1):
                if kept[j - sp, sp] and (mask[d - sp, i] & UB_1):
                    out.add((i, j - sp, j))
    return out


def popcount(words):
    return sum(bin(int(w)).count("1") for w in words[np.nonzero(words)])


@pytest.mark.parametrize("C", [30, 5])
@pytest.mark.parametrize("pattern", [P1, P5])
def test_host_entry_equals_the_restatement_and_both_words_hold_the_same_triples(pattern, C, capsys):
    lines = []
    for k, (name, seq) in enumerate(CASES):
        kept = kept_of(pattern, C, k)
        L, W = kept.shape[0] - 1, kept.shape[1] - 1
        mask = api.useful_mask_host(kept, max_iloop=C)
        ha, h1 = api.pair_terms_host(mask, kept)
        assert ha.shape == h1.shape == (W + 1, L + 1) and ha.dtype == h1.dtype == np.uint64
        want_ha, want_h1 = numpy_words(mask, kept)
        assert np.array_equal(ha, want_ha), "%s: ha_rows differs from the restatement at (d, i) = %s" % (name, tuple(np.argwhere(ha != want_ha)[0]))
        assert np.array_equal(h1, want_h1), "%s: h1_stems differs from the restatement at (d, i) = %s" % (name, tuple(np.argwhere(h1 != want_h1)[0]))
        # words only at kept pairs / at parsable cells with UB_1, and no bit past the span
        assert not ha[kept.T == 0].any() and not h1[(mask & UB_1) == 0].any(), name
        for words in (ha, h1):
            for d in range(W + 1):
                assert not (words[d] >> np.uint64(min(W - d, 63))).any(), (name, d)
        t_ha, t_h1 = triples_ha(ha), triples_h1(h1)
        assert t_ha == t_h1, "%s: %d triples in ha_rows, %d in h1_stems" % (name, len(t_ha), len(t_h1))
        assert t_ha == triples_inside(mask, kept), name
        if L == 200:
            ok_ha, ok_h1 = api.pair_terms_host(np.full_like(mask, 255), kept)
            n_ok, n_ha, n_st, n_h1 = popcount(ok_ha), popcount(ha), popcount(ok_h1), popcount(h1)
            slots = sum(W - d for d, i in zip(*np.nonzero(kept.T)))
            lines.append("%-10s %s C %2d kept pairs %4d | HA slots %6d, ok %6d, useful %6d | H1 stems of left_ok cells %6d, useful %6d" % (
                name, pattern, C, int(kept.sum()), slots, n_ok, n_ha, n_st, n_h1))
            assert 0 < n_ha < n_ok <= slots and 0 < n_h1 == n_ha, name      # the words drop something
    with capsys.disabled():
        print()
        print("\n".join(lines))


def test_no_kept_pair_gives_no_word():
    kept = np.zeros((61, 51), dtype=np.uint8)
    for mask in (api.useful_mask_host(kept, max_iloop=30), np.full((51, 61), 255, dtype=np.uint8)):
        ha, h1 = api.pair_terms_host(mask, kept)
        assert not ha.any() and not h1.any()


@pytest.mark.parametrize("k", [0, 2])
def test_mask_of_all_ones_gives_the_rows_and_stems_walked_without_words(k):
    """ha_rows = the rows that pass the kernel's `ok` (i - b >= 0, dmin[i - b] > 0, b >= dmin[i - b]) of every kept pair; h1_stems =
    the kept pairs that start at the end of every parsable cell, up to the span"""
    kept = kept_of(P1, 30, k)
    L, W = kept.shape[0] - 1, kept.shape[1] - 1
    dmin = dmin_of(kept)
    ha, h1 = api.pair_terms_host(np.full((W + 1, L + 1), 255, dtype=np.uint8), kept)
    for d in range(W + 1):
        for i in range(L - d + 1):
            rows = [b - 1 for b in range(1, W - d + 1) if i - b >= 0 and 0 < dmin[i - b] <= b] if kept[i, d] else []
            assert bits_of(ha[d, i]) == rows, (d, i)
            j = i + d
            stems = [sp - 1 for sp in range(1, min(W - d, L - j) + 1) if kept[j, sp]] if 0 < dmin[i] <= d else []
            assert bits_of(h1[d, i]) == stems, (d, i)


def test_span_64_fills_the_word_and_65_is_refused():
    """W = 64: the longest rows and stems a kept pair of span d >= 1 can have use bit 62; bit 63 belongs to d = 0, which no filter
    keeps -- a kept[i, 0] set by hand reaches it, so the top bit of the word is whole.  W = 65 has no words."""
    L, W = 80, 64
    kept = np.zeros((L + 1, W + 1), dtype=np.uint8)
    kept[70, 1] = kept[6, 64] = kept[6, 1] = kept[7, 63] = 1       # rows of (70, 1) down to b = 63 <-> stem (7, 63) behind (6, 1)
    kept[72, 0] = kept[8, 64] = 1                                    # the hand-made d = 0 pair and its row b = 64
    ones = np.full((W + 1, L + 1), 255, dtype=np.uint8)
    ha, h1 = api.pair_terms_host(ones, kept)
    want_ha, want_h1 = numpy_words(ones, kept)
    assert np.array_equal(ha, want_ha) and np.array_equal(h1, want_h1)
    assert (int(ha[1, 70]) >> 62) & 1 and bits_of(ha[63, 7]) == [0] and 62 in bits_of(h1[1, 6])
    assert (int(ha[0, 72]) >> 63) & 1
    assert (8, 72, 72) in triples_ha(ha)
    assert {t for t in triples_ha(ha) if t[1] != t[2]} == triples_h1(h1)      # (a stem of span 0 has no left cell's bit)
    lib = api.load_library()
    k65, m65 = np.zeros((L + 1, 66), dtype=np.uint8), np.zeros((66, L + 1), dtype=np.uint8)
    w65 = np.zeros((66, L + 1), dtype=np.uint64)
    assert lib.elemdp_pair_terms_host(api._u8(m65), api._u8(k65), L, 65, api._u64(w65), api._u64(w65)) < 0
    with pytest.raises(api.ElemdpError):
        api.pair_terms_host(m65, k65)
    assert lib.elemdp_pair_terms_host(None, api._u8(kept), L, W, api._u64(ha), api._u64(h1)) < 0
