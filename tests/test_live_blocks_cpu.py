"""The live-block lists of the train sweeps without a GPU: the host entry elemdp_live_blocks_host, which
runs the rule function of rnaelem_amd/csrc/live_blocks.h that the plan kernel runs, against a NumPy restatement of the rule in
this file, and against the properties the band kernels rely on: every live cell in exactly one block, ascending; no dead cell in
any; the owned ranges partition the diagonal; no more blocks than the grid of consecutive blocks has.

The masks come from elemdp_useful_mask_host on the cases of tests/test_useful_mask_cpu.py (plus the other sequences of its
synthetic draws, so that three sequences of L = 37 and of L = 60 are in), an all-ones and an all-zero mask.  The counts of blocks
with gaps and of blocks closed by the span are printed (pytest -s)."""
import numpy as np
import pytest

from oracle import pyoracle as po
from rnaelem_amd import api, synth
from tests.test_useful_mask_cpu import CASES

PARAMS = [(12, 12), (12, 16), (12, 24), (12, 32), (18, 18), (18, 24), (18, 32)]      # (cpb, cap)


def numpy_blocks(mask, cpb, cap):
    """the rule, restated: per diagonal the blocks (first cell, [live cells], (own_lo, own_end))"""
    W, L = mask.shape[0] - 1, mask.shape[1] - 1
    out = []
    for d in range(W + 1):
        ncell, blocks = L - d + 1, []
        for i in [i for i in range(max(ncell, 0)) if mask[d, i]]:
            if not blocks or len(blocks[-1]) == cpb or i - blocks[-1][0] >= cap:
                blocks.append([i])
            else:
                blocks[-1].append(i)
        first = [b[0] for b in blocks] + [ncell]
        out.append([(b[0], b, (0 if k == 0 else b[0], first[k + 1])) for k, b in enumerate(blocks)])
    return out


def masks():
    out = []
    seqs = [(name, seq) for name, seq in CASES]
    for L in (37, 60):
        draw = synth.synth_codes(3, L)
        seqs += [("synth L%d #%d" % (L, k), draw[k]) for k in (0, 2)]
    for name, seq in seqs:
        o = po.make_oracle("((.*.))", 50, 30, min_bpp=1e-4, tau=0.1, lam=(1.0, 1.0))
        _, kept, _, _ = o.bpp(seq)
        out.append((name, api.useful_mask_host(kept, max_iloop=30)))
    ones = np.zeros((51, 131), dtype=np.uint8)
    dd, ii = np.meshgrid(np.arange(51), np.arange(131), indexing="ij")
    ones[ii + dd <= 130] = 255
    out.append(("all ones L130", ones))
    out.append(("all zero L60", np.zeros((51, 61), dtype=np.uint8)))
    return out


MASKS = masks()


def count_kinds(lists, cpb):
    """(blocks, blocks whose live cells are not consecutive, blocks closed by the span: short of cpb cells, yet not the last)"""
    n = gaps = capped = 0
    for row in lists:
        for k, (first, cells, _) in enumerate(row):
            n += 1
            gaps += cells[-1] - first + 1 > len(cells)
            capped += len(cells) < cpb and k + 1 < len(row)
    return n, gaps, capped


@pytest.mark.parametrize("cpb,cap", PARAMS)
def test_host_lists_follow_the_rule(cpb, cap, capsys):
    lines, total = [], {}
    for name, mask in MASKS:
        W, L = mask.shape[0] - 1, mask.shape[1] - 1
        got = api.live_blocks_host(mask, cpb, cap)
        assert got == numpy_blocks(mask, cpb, cap), "%s: host entry differs from the NumPy restatement" % name
        assert len(got) == W + 1
        for d, row in enumerate(got):
            ncell = L - d + 1
            listed = [i for _, cells, _ in row for i in cells]
            assert listed == [i for i in range(ncell) if mask[d, i]], (name, d)       # every live cell once, ascending, no dead one
            assert len(row) <= (ncell + cpb - 1) // cpb, (name, d)
            for first, cells, _ in row:
                assert cells[0] == first and len(cells) <= cpb and cells[-1] - first < cap, (name, d)
            owned = [r for _, _, r in row]
            if row:                                                                   # the owned ranges partition 0 .. ncell - 1
                assert owned[0][0] == 0 and owned[-1][1] == ncell, (name, d)
                assert all(a[1] == b[0] for a, b in zip(owned, owned[1:])), (name, d)
                assert all(lo <= first < hi for (first, _, _), (lo, hi) in zip(row, owned)), (name, d)
            else:
                assert not mask[d, :max(ncell, 0)].any(), (name, d)
        n, gaps, capped = count_kinds(got, cpb)
        key = "L%d" % L
        t = total.setdefault(key, [0, 0, 0])
        t[0] += n; t[1] += gaps; t[2] += capped
        lines.append("%-16s cpb %2d cap %2d: %4d blocks, %3d with gaps, %3d closed by the span" % (name, cpb, cap, n, gaps, capped))
    # the inputs reach both branches of the rule
    assert total["L37"][1] > 0 and total["L60"][1] > 0, total
    if cap == 16:
        assert total["L60"][2] > 0, total
    if cap == 32 and cpb == 12:
        assert total["L200"][2] > 0, total
    with capsys.disabled():
        print()
        print("\n".join(lines))


def test_all_ones_mask_gives_consecutive_blocks():
    name, mask = MASKS[-2]
    for cpb, cap in PARAMS:
        for d, row in enumerate(api.live_blocks_host(mask, cpb, cap)):
            ncell = 130 - d + 1
            assert [cells for _, cells, _ in row] == [list(range(i, min(i + cpb, ncell))) for i in range(0, ncell, cpb)]


def test_all_zero_mask_has_no_block():
    assert all(row == [] for row in api.live_blocks_host(MASKS[-1][1], 12, 32))


def test_span_below_the_block_size_is_refused():
    mask = MASKS[0][1]
    with pytest.raises(api.ElemdpError):
        api.live_blocks_host(mask, 12, 11)
    with pytest.raises(api.ElemdpError):
        api.live_blocks_host(mask, 18, 16)
    with pytest.raises(api.ElemdpError):
        api.live_blocks_host(mask, 12, 65)      # (beyond the 64 cells a record can list)
