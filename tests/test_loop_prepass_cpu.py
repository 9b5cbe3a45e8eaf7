"""The lists of the inside sweep behind the loop pre-pass (option loop_prepass) without a GPU: the host
entry elemdp_live_blocks_host_bits, which runs the rule function of rnaelem_amd/csrc/live_blocks.h that the plan kernel runs, with
the bits of the inside set (every mask bit but L) against a plain NumPy restatement of the rule, on the cases of
tests/test_useful_mask_cpu.py (both patterns, L = 37 / 60 / 200, N bases, poly-A, tiny.fq; C = 30 and 5); the rule with all bits
against the present host entry; and the premise of the skipped launches: no bit other than L on a diagonal d + 2 < min_span."""
import numpy as np
import pytest

from oracle import pyoracle as po
from rnaelem_amd import api
from tests.test_useful_mask_cpu import BIT, CASES, P1, P5

MIN_SPAN = 5
GEOMETRIES = [(12, 32), (12, 12), (8, 64), (16, 16)]        # (cells per block, span): the bench's, no slack, the extremes


def numpy_lists(mask, cpb, cap, bits):
    """live_blocks_row, restated: the cells of a diagonal whose byte has one of `bits`, in ascending order; a block takes the
    next one until it holds cpb of them or the next lies cap or more cells behind its first; a block owns the cells from its first
    live cell to the next block's first, the first block also those in front, the last those behind"""
    W, L = mask.shape[0] - 1, mask.shape[1] - 1
    out = []
    for d in range(W + 1):
        ncell = L - d + 1
        live = [i for i in range(ncell) if int(mask[d, i]) & bits]
        groups = []
        for i in live:
            if not groups or len(groups[-1]) == cpb or i - groups[-1][0] >= cap:
                groups.append([])
            groups[-1].append(i)
        row = []
        for b, cells in enumerate(groups):
            lo = 0 if b == 0 else cells[0]
            end = groups[b + 1][0] if b + 1 < len(groups) else ncell
            row.append((cells[0], cells, (lo, end)))
        out.append(row)
    return out


_KEPT = {}


def kept_pairs(pattern, C, name, seq):
    """the oracle's kept pairs (they depend on neither the pattern nor C: one filter run per sequence)"""
    if name not in _KEPT:
        _KEPT[name] = po.make_oracle(pattern, 50, C, min_bpp=1e-4, tau=0.1, lam=(1.0, 1.0)).bpp(seq)[1]
    return _KEPT[name]


@pytest.mark.parametrize("C", [30, 5])
@pytest.mark.parametrize("pattern", [P1, P5])
def test_inside_lists_against_the_numpy_restatement(pattern, C):
    n_less = 0
    for name, seq in CASES:
        mask = api.useful_mask_host(kept_pairs(pattern, C, name, seq), max_iloop=C)
        for cpb, cap in GEOMETRIES:
            got = api.live_blocks_host(mask, cpb, cap, bits=api.LIVE_INSIDE_BITS)
            assert got == numpy_lists(mask, cpb, cap, api.LIVE_INSIDE_BITS), (name, cpb, cap)
            # the rule with all bits is the present host entry, and the NumPy restatement of that
            whole = api.live_blocks_host(mask, cpb, cap, bits=255)
            assert whole == api.live_blocks_host(mask, cpb, cap) == numpy_lists(mask, cpb, cap, 255), (name, cpb, cap)
            n_in, n_all = sum(len(r) for r in got), sum(len(r) for r in whole)
            assert n_in <= n_all, (name, cpb, cap)
            n_less += n_in < n_all
            # the owned ranges of a diagonal with a block partition its cells
            L = mask.shape[1] - 1
            for d, row in enumerate(got):
                if row:
                    assert row[0][2][0] == 0 and row[-1][2][1] == L - d + 1, (name, d)
                    assert all(a[2][1] == b[2][0] for a, b in zip(row, row[1:])), (name, d)
    assert n_less > 0          # (the L plane keeps cells alive that nothing else does: the inside set is smaller somewhere)


@pytest.mark.parametrize("C", [30, 5])
def test_no_entry_outside_the_loop_plane_below_the_first_hairpin(C):
    """E(i, d) closes a pair of span d + 2 >= min_span, every other plane needs a span >= min_span: the diagonals d + 2 < min_span
    hold L bits only -- the launches the inside sweep drops -- and no block of the inside lists"""
    some_l = False
    for name, seq in CASES:
        mask = api.useful_mask_host(kept_pairs(P1, C, name, seq), max_iloop=C)
        low = mask[:MIN_SPAN - 2]
        assert not (low & api.LIVE_INSIDE_BITS).any(), name
        some_l = some_l or bool((low & BIT["L"]).any())
        lists = api.live_blocks_host(mask, 12, 32, bits=api.LIVE_INSIDE_BITS)
        assert all(row == [] for row in lists[:MIN_SPAN - 2]), name
    assert some_l              # (... while the whole-byte lists do have blocks there)


def test_host_entry_rejects_bad_arguments():
    lib = api.load_library()
    mask = np.zeros((11, 11), dtype=np.uint8)
    counts = np.zeros(11, dtype=np.int32)
    recs = np.zeros((11, 2), dtype=api.LIVE_BLOCK)
    ip = counts.ctypes.data_as(api.C.POINTER(api.C.c_int32))
    rp = recs.ctypes.data_as(api.C.c_void_p)
    assert lib.elemdp_live_blocks_host_bits(api._u8(mask), 10, 10, 12, 32, 127, ip, rp, 2) == 0
    assert lib.elemdp_live_blocks_host_bits(api._u8(mask), 10, 10, 12, 32, 0, ip, rp, 2) < 0       # no bit
    assert lib.elemdp_live_blocks_host_bits(api._u8(mask), 10, 10, 12, 32, 256, ip, rp, 2) < 0
    assert lib.elemdp_live_blocks_host_bits(api._u8(mask), 10, 10, 12, 8, 127, ip, rp, 2) < 0      # cap < cpb
    assert lib.elemdp_live_blocks_host_bits(None, 10, 10, 12, 32, 127, ip, rp, 2) < 0
