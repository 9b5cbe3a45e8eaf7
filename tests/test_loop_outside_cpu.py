"""The rule functions of the outside L plane behind the sweep (option loop_outside; lin_fast.h:
loop_outside_seed_term, loop_outside_entry, fast_outside_unary with LPOST) without a GPU: the test-only driver
tests/loop_outside_emul.cpp runs pass 0 of the reference schedule the way the GPU does with the option on -- the sweep without any
L work, then seeds and chain cell by cell over NaN-filled tables -- for the sequences of L = 37 and 60 of
tests/test_useful_mask_cpu.py and one of L = 7.
Checked: the outside L plane against the oracle wherever both are finite (rtol 1e-10 on the logs, the bound of the other table
comparisons of the emulation with the oracle; d >= 1: the table-driven forms leave the rule-6c sums of the empty loops L(i, i) out,
whose outside value has no reader) and against the emulation's parent path (fast_outside_cell, every entry of every diagonal);
the expected counts and the energy statistics of the pass, which hold the L <- L counts and the 6b statistic of the chain,
against the oracle's and the parent path's (rtol 1e-9 / atol 1e-11, the bound of tests/test_round4_cpu.py for the same numbers:
the oracle does not expose the L-transition counts apart from the others)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from oracle import pyoracle as po
from tests.emul import build as _emul_build
from tests.emul.pyemul import Emul
from tests.test_emul_vs_oracle import PAR, useful_mask
from tests.test_useful_mask_cpu import CASES as MASK_CASES
from tests.util import assert_log_close

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "loop_outside_emul.cpp")
LIB = os.path.join(HERE, "libloop_outside_emul.so")
ST_L = 6
PATTERN = "((.*.))"
_lib = None


def driver():
    global _lib
    if _lib is None:
        srcs = [SRC] + _emul_build.SRCS[1:]
        deps = [SRC] + _emul_build.DEPS
        if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in deps):
            subprocess.check_call(["g++", "-std=c++14", "-O2", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-o", LIB] + srcs)
        L = C.CDLL(LIB)
        dp, u8 = C.POINTER(C.c_double), C.POINTER(C.c_uint8)
        L.emu_create.restype = C.c_void_p
        L.emu_create.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int]
        L.emu_destroy.argtypes = [C.c_void_p]
        L.emu_last_error.restype = C.c_char_p
        L.emu_set_prune.argtypes = [C.c_void_p, C.c_int]
        L.emu_set_fast.argtypes = [C.c_void_p, C.c_int]
        L.emu_n_param.argtypes = [C.c_void_p]
        L.emu_n_state.argtypes = [C.c_void_p]
        L.emu_loop_outside_seq.argtypes = [C.c_void_p, dp, u8, C.c_int, u8, dp, dp, dp]
        _lib = L
    return _lib


def sequences():
    """L = 7 (GC AAA GC: the first hairpin), and the synthetic sequences of L = 37 and 60 of the mask tests"""
    enc = {"A": 1, "C": 2, "G": 3, "U": 4}
    out = [np.array([enc[c] for c in "GCAAAGC"], dtype=np.uint8)]
    by_name = dict(MASK_CASES)
    return out + [np.asarray(by_name["synth L%d" % L], dtype=np.uint8) for L in (37, 60)]


@pytest.fixture(scope="module")
def setup():
    o = po.make_oracle(PATTERN, 50, 30, min_bpp=1e-4, tau=0.1)
    e = Emul(PATTERN, PAR, 50, 30, 1e-4, 0.1, 0)
    e.set_prune(True)
    assert e.set_fast(1) & 1
    x = np.zeros(e.n_param)
    x[:-2] = -1.4 + np.linspace(-0.3, 0.3, e.n_param - 2)
    x[-2:] = (1.0, 0.7)
    o.set_params(x)
    D = driver()
    h = D.emu_create(PATTERN.encode(), PAR.encode(), 50, 30, 1e-4, 0.1, 0)
    assert h, D.emu_last_error()
    D.emu_set_prune(h, 1)
    assert D.emu_set_fast(h, 1) & 1
    yield o, e, x, D, h
    D.emu_destroy(h)


@pytest.mark.parametrize("k", [0, 1, 2], ids=["L7", "L37", "L60"])
def test_seed_and_chain_rules_give_the_outside_l_plane_and_its_statistics(setup, k):
    o, e, x, D, h = setup
    seq = sequences()[k]
    L, W, S = len(seq), min(len(seq), 50), e.S
    qual = np.full(L + 1, 10, dtype=np.uint8)
    qual[-1] = 0
    a = o.train_seq(seq, qual, tables=True)
    b = e.train_seq(x, seq, qual, tables=True, linear=0)            # the emulation's parent path (table-driven forms)
    assert not a["skipped"] and b["skipped"] == 0
    nt = e.n_param - 2
    EN, EH, outL = np.zeros(nt), np.zeros(2), np.full((L + 1) * (W + 1) * S, np.nan)
    dp, u8 = C.POINTER(C.c_double), C.POINTER(C.c_uint8)
    rc = D.emu_loop_outside_seq(h, x.ctypes.data_as(dp), seq.ctypes.data_as(u8), L, qual.ctypes.data_as(u8), EN.ctypes.data_as(dp),
                                EH.ctypes.data_as(dp), outL.ctypes.data_as(dp))
    assert rc == 0, D.emu_last_error()
    outL = outL.reshape(L + 1, W + 1, S)
    assert not np.isnan(outL).any() and np.all(np.isfinite(EN)) and np.all(np.isfinite(EH))
    # against the emulation's parent path: every entry
    assert_log_close(outL, b["outside"][:, :, ST_L, :], rtol=1e-10, what="outside L against the parent path")
    # against the oracle: the useful states of the plane, wherever both are finite
    um = useful_mask(e)[ST_L]
    want = a["outside"][:, 1:, ST_L, :][:, :, um]
    got = outL[:, 1:, um]
    both = np.isfinite(want) & np.isfinite(got)
    print("L %d: %d outside L entries finite in both, %d in the oracle alone, %d here alone" % (
        L, int(both.sum()), int((np.isfinite(want) & ~both).sum()), int((np.isfinite(got) & ~both).sum())))
    assert both.sum() > 0
    assert_log_close(got[both], want[both], rtol=1e-10, what="outside L against the oracle")
    for name, have, ref in (("EN", EN, b["ENo"]), ("EH", EH, b["EHo"]), ("EN", EN, a["ENo"]), ("EH", EH, a["EHo"])):
        np.testing.assert_allclose(have, ref, rtol=1e-9, atol=1e-11, err_msg=name)
