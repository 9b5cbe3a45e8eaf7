"""The slot sizing arithmetic (rnaelem_amd/csrc/slot_sizing.h) against a restatement of what the engine computed before the
arithmetic had a place of its own (Engine::ensure_slots and Engine::balanced_group, written out below with the wrap-around of
size_t, the casts and the double products of the C++).  The functions run in tests/slots_check.cpp, a stand-alone program built
with -fsanitize=address,undefined that must also end clean; all results are integers and are compared exactly."""
import itertools
import os
import subprocess
from collections import Counter

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "rnaelem_amd", "csrc")
SRC = os.path.join(HERE, "slots_check.cpp")
EXE = os.path.join(HERE, "slots_check_asan")
M64 = 1 << 64
TRACE_REC = 8       # sizeof(TraceRec), device_layout.h
GB = 1 << 30


def u64(x):
    return x % M64


def cast(x, bits):
    x %= 1 << bits
    return x - (1 << bits) if x >> (bits - 1) else x


def frac(x, f):
    """(size_t)((double)x * f)"""
    return int(float(x) * f)


# ---- the arithmetic as it stood -----------------------------------------------------------------------------------------------------

def old_ensure_slots(S, row, scan, n_want, override, opt_slots, n_cu, Lmax, Wmax, au_S, slot_budget, free, held, have, tags):
    """(want, band, ext, dense1, per_slot, keep, sized): `sized` is the slot count of a fresh sizing, 0 for 'not enough device
    memory for one table slot'; `have` = (count, S, band stride, sized by a scan) of the slots that are there"""
    row_given = row > 0
    if row <= 0:
        row = 7 * S
    band = u64((Wmax + 1) * (Lmax + 1) * row)
    dense1 = u64(7 * (Wmax + 1) * (Lmax + 1) * au_S)
    ext = u64((Lmax + 1) * S)
    want = opt_slots if opt_slots > 0 else 2 * n_cu
    src = "slots" if opt_slots > 0 else "cap"
    if override > 0:
        want, src = override, "group"
    if n_want < want:
        src = "n_want"
    want = max(1, min(want, n_want))
    tags["want:" + src] += 1
    per_slot = u64(u64(band + ext) * 2 * 8 + (u64(ext * TRACE_REC) + 16 * (Lmax + 2) if scan else 0))
    tags["per_slot:" + ("scan" if scan else "train")] += 1
    hn, hS, hband, hscan = have
    keep = hn >= want and hS == S and hband == band and (hscan or not scan)
    if hn > 0:
        if keep:
            tags["keep:larger" if hn > want else "keep:same"] += 1
        elif hn < want:
            tags["discard:fewer"] += 1
        elif hS != S:
            tags["discard:S"] += 1
        elif hband != band:
            tags["discard:row" if row_given else "discard:band"] += 1
        else:
            tags["discard:trace"] += 1
    want0 = want
    reach = u64(free + held)
    budget = frac(reach, 0.72)
    inner = slot_budget > 0 and slot_budget < budget
    if slot_budget > 0:
        budget = min(budget, slot_budget)
    if u64(per_slot * want) > budget:
        want = cast(max(1, budget // per_slot), 32)
        tags["cut:inner" if inner else "cut:budget"] += 1
        if budget // per_slot == 0:
            tags["floor:one"] += 1
    if u64(per_slot * u64(want)) > reach:
        tags["refuse"] += 1
        want = 0
    return want0, band, ext, dense1, per_slot, int(keep), want


def old_balanced_group(per_slot_bytes, n, group_cap, opt_group, slot_budget, free, held, tags):
    if opt_group > 0:
        tags["group:option"] += 1
        return opt_group
    budget = frac(u64(free + held), 0.68)
    if slot_budget > 0:
        tags["group:inner" if slot_budget < budget else "group:inner_loose"] += 1
        budget = min(budget, slot_budget)
    cap = cast(budget // max(per_slot_bytes, 1), 64)
    tags["group:cap" if cap >= group_cap else "group:memory" if cap >= 1 else "group:floor"] += 1
    cap = max(1, min(cap, group_cap))
    n_groups = (n + cap - 1) // cap
    return cast((n + n_groups - 1) // n_groups, 32)


def old_rebalance(n_need, n_slots):
    """prepare_lin and the ranged evaluation of run_lin_batch: the group size for the slots the allocation gave"""
    n_groups = (n_need + n_slots - 1) // n_slots
    return (n_need + n_groups - 1) // n_groups


def old_lin_bytes(Lmax, Wmax, row, Sa, nap):
    """prepare_lin: the per_slot_bytes it hands to balanced_group"""
    cells, ext = u64((Wmax + 1) * (Lmax + 1)), Lmax + 1
    return u64(u64(cells * row + ext * Sa) * 2 * 8 + ext * Sa * 3 * 8 + cells * nap * 2 * 8)


# ---- the cases -----------------------------------------------------------------------------------------------------------------------

def slot_cases():
    """(line of the driver, arguments of old_ensure_slots)"""
    shapes = [(200, 50, 29, 7, 28), (300, 50, 29, 0, 28), (60, 50, 5, 13, 4), (1, 1, 1, 0, 1), (90, 30, 128, 64, 127)]
    for (Lmax, Wmax, S, row, au_S), scan, n_want, (override, opt_slots), slot_budget in itertools.product(
            shapes, (0, 1), (1, 3, 128, 10000), ((0, 0), (0, 3), (0, 700), (4096, 0), (2, 5), (1000, 0)), (0, 1, 3 * GB)):
        n_cu = 256
        band = (Wmax + 1) * (Lmax + 1) * (row if row > 0 else 7 * S)
        per = (band + (Lmax + 1) * S) * 16 + (((Lmax + 1) * S * TRACE_REC + 16 * (Lmax + 2)) if scan else 0)
        want = max(1, min(override or opt_slots or 2 * n_cu, n_want))
        haves = [(0, 0, 0, 0), (want, S, band, scan), (want + 5, S, band, 1), (want - 1, S, band, 1), (want, S + 1, band, 1),
                 (want, S, band + (Wmax + 1) * (Lmax + 1), 1), (want, S, band, 0)]
        mems = [(0, 0), (per - 1, 0), (per, 0), (per + per // 5, 0), (per, per), (3 * per, 0), (per * want // 2, per * want),
                (per * want * 2, 0), (288 * GB, 0), (200 * GB, 60 * GB)]
        for k, (free, held) in enumerate(mems):
            have = haves[k % len(haves)] if (scan + n_want + override + opt_slots) % 2 else haves[(k + 3) % len(haves)]
            yield case_line(S, row, scan, n_want, override, opt_slots, n_cu, Lmax, Wmax, au_S, slot_budget, free, held, have)
    # the edges: products near 2^63 and past 2^64, no memory at all, all of it
    big = (1 << 30) - 1
    for Lmax, Wmax, S, row in ((big, big, 1, 0), (big, big, 3, 1), (big, 1 << 28, 128, 900), (big, 3, 64, 0), (1 << 20, 1 << 20, 128, 0)):
        for scan, n_want, override, free, held, slot_budget in itertools.product(
                (0, 1), (1, (1 << 31) - 1), (0, (1 << 31) - 1), (0, (1 << 63) - 1, (1 << 63) + 12345, M64 - 1), (0, 1 << 62, M64 - 1),
                (0, (1 << 63) + 1)):
            yield case_line(S, row, scan, n_want, override, 0, 256, Lmax, Wmax, S, slot_budget, free, held, (7, S, 1 << 62, scan))


def case_line(S, row, scan, n_want, override, opt_slots, n_cu, Lmax, Wmax, au_S, slot_budget, free, held, have):
    pair_row = 0   # (sizes the pair tables only: no part of the slot count)
    vals = (S, row, scan, n_want, override, opt_slots, n_cu, pair_row, Lmax, Wmax, au_S, slot_budget, free, held) + tuple(have)
    return "S " + " ".join(str(int(v)) for v in vals), (S, row, scan, n_want, override, opt_slots, n_cu, Lmax, Wmax, au_S,
                                                        slot_budget, free, held, have)


def group_cases():
    pers = [old_lin_bytes(200, 50, 64, 29, 12), old_lin_bytes(300, 50, 203, 29, 12), old_lin_bytes(60, 50, 9, 5, 0), 1, 0]
    for per, n, cap, opt_group, slot_budget, (free, held) in itertools.product(
            pers, (1, 2, 128, 1100, 10000), (8192, 1024, 1), (0, 2, 64), (0, 1, 2 * GB, 1 << 50),
            ((0, 0), (1, 0), (100 * GB, 0), (280 * GB, 5 * GB), (M64 - 1, 0), ((1 << 63) - 1, 1 << 63), (M64 - 1, M64 - 1))):
        yield "G %d %d %d %d %d %d %d" % (per, n, cap, opt_group, slot_budget, free, held), (per, n, cap, opt_group, slot_budget, free, held)


@pytest.fixture(scope="module")
def exe():
    deps = [SRC, os.path.join(CSRC, "slot_sizing.h"), os.path.join(CSRC, "device_layout.h")]
    if not os.path.exists(EXE) or any(os.path.getmtime(d) > os.path.getmtime(EXE) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-o", EXE, SRC])
    return EXE


def run(exe, lines):
    # (the program allocates nothing of its own: the leak check, which some sandboxes cannot start, is left out)
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-2000:])
    out = r.stdout.split("\n")[:-1]
    assert len(out) == len(lines)
    return out


def test_slot_counts_are_what_ensure_slots_computed(exe):
    cases = list(slot_cases())
    out = run(exe, [c[0] for c in cases])
    tags = Counter()
    for (line, args), got in zip(cases, out):
        assert tuple(int(v) for v in got.split()) == old_ensure_slots(*args, tags), line
    print(len(cases), "cases;", dict(tags))
    for branch in ("want:n_want", "want:cap", "want:slots", "want:group", "per_slot:scan", "per_slot:train", "cut:budget", "cut:inner",
                   "floor:one", "refuse", "keep:larger", "keep:same", "discard:fewer", "discard:S", "discard:row", "discard:band",
                   "discard:trace"):
        assert tags[branch] > 0, branch


def test_group_sizes_are_what_balanced_group_computed(exe):
    cases = list(group_cases())
    out = run(exe, [c[0] for c in cases])
    tags = Counter()
    for (line, args), got in zip(cases, out):
        assert int(got) == old_balanced_group(*args, tags), line
    print(len(cases), "cases;", dict(tags))
    for branch in ("group:option", "group:inner", "group:inner_loose", "group:cap", "group:memory", "group:floor"):
        assert tags[branch] > 0, branch


def test_rebalanced_groups_and_group_bytes(exe):
    pairs = [(n, s) for n in (1, 2, 3, 5, 64, 128, 1100, 2500, 10000, (1 << 31) - 1) for s in (1, 2, 3, 64, 512, 1024, 4096, (1 << 31) - 1)]
    shapes = [(200, 50, 64, 29, 12), (300, 50, 203, 30, 0), (1, 1, 1, 1, 1), ((1 << 30) - 1, (1 << 30) - 1, 900, 128, 500)]
    out = run(exe, ["E %d %d" % p for p in pairs] + ["B %d %d %d %d %d" % s for s in shapes])
    assert [int(v) for v in out[:len(pairs)]] == [old_rebalance(*p) for p in pairs]
    assert [int(v) for v in out[len(pairs):]] == [old_lin_bytes(*s) for s in shapes]
