"""Maximum expected accuracy structures under the motif model, host side: the host mirror of the rule
against a brute-force maximum, the record format of `scan --out-mea`, the command line, the sharded writer, the exported symbol."""
import re

import numpy as np
import pytest

from rnaelem_amd import api, cli, io
from tests.mea_mirror import expected_accuracy, mea_fold, pairs_of
from tests.test_host_abi import HEADER


def all_structures(L, kept):
    """every nested structure on [0, L) whose pairs are kept cells (i, d), d >= 2"""
    memo = {}

    def sub(a, b):      # structures of [a, b)
        if (a, b) in memo:
            return memo[(a, b)]
        if a >= b:
            return [""]
        out = ["." + s for s in sub(a + 1, b)]
        for d in range(2, min(b - a, kept.shape[1] - 1) + 1):
            if kept[a, d]:
                out += ["(" + s + ")" + t for s in sub(a + 1, a + d - 1) for t in sub(a + d, b)]
        memo[(a, b)] = out
        return out

    return sub(0, L)


@pytest.mark.parametrize("seed", range(12))
def test_mirror_attains_the_brute_force_maximum(seed):
    rng = np.random.default_rng(seed)
    L = int(rng.integers(1, 13))
    W = int(rng.integers(1, L + 1))
    kept = rng.random((L + 1, W + 1)) < 0.45
    kept[:, :2] = False
    for i in range(L + 1):
        kept[i, L - i + 1:] = False
    P = np.where(kept, rng.random((L + 1, W + 1)) * 0.5, 0.0)
    if seed % 3 == 0:       # (ties: a few equal weights)
        P = np.where(kept, np.round(P * 4) / 8, 0.0)
    q = rng.random(L)
    for gamma in (0.3, 1.0, 4.0):
        s, score = mea_fold(P, kept, q, gamma)
        assert len(s) == L
        assert all(kept[i, d] for i, d in pairs_of(s))
        best = max(expected_accuracy(t, P, q, gamma) for t in all_structures(L, kept))
        assert score == pytest.approx(best, rel=1e-12, abs=1e-12)
        assert expected_accuracy(s, P, q, gamma) == pytest.approx(best, rel=1e-12, abs=1e-12)


def test_mirror_without_kept_pairs_leaves_every_base_unpaired():
    L = 7
    s, score = mea_fold(np.zeros((L + 1, 4)), np.zeros((L + 1, 4), dtype=bool), np.ones(L), 1.0)
    assert s == "......." and score == 7.0


def test_mea_record_formats_and_parses_back(tmp_path):
    text = io.mea_record("@r1", "((..))..", 7.123456789012345678)
    assert text == "id: @r1\nmea: ((..))..\nscore: %.17g\n" % 7.123456789012345678
    empty = io.mea_record("@r2", "", 0.0)
    assert empty == "id: @r2\nmea: \nscore: 0\n"
    path = tmp_path / "m.txt"
    path.write_text(text + io.mea_record("@r3", "...", 3.0) + empty)
    recs = io.read_mea_records(str(path))
    assert recs == [("@r1", "((..))..", 7.123456789012345678), ("@r3", "...", 3.0), ("@r2", "", 0.0)]


def test_scan_parser_accepts_the_mea_options():
    a = cli.build_parser().parse_args(["scan", "-f", "x.fq", "-q", "m.txt", "--out1", "a.raw", "--out-mea", "m.txt",
                                       "--mea-gamma", "4"])
    assert a.out_mea == "m.txt" and a.mea_gamma == 4.0
    a = cli.build_parser().parse_args(["scan", "-f", "x.fq", "-q", "m.txt", "--out1", "a.raw"])
    assert a.out_mea is None and a.mea_gamma == 1.0


def test_sharded_writer_of_one_rank_writes_three_files(tmp_path):
    recs = [("@r%d" % k, None, None) for k in range(4)]
    outs = [str(tmp_path / n) for n in ("scan.raw", "pairs.txt", "mea.txt")]

    def part(mine):
        for rid, _, _ in mine:
            yield "scan %s\n" % rid, "pairs %s\n" % rid, "mea %s\n" % rid

    cli.sharded_write(recs, outs, 0, 1, part, lambda: None)
    for o, tag in zip(outs, ("scan", "pairs", "mea")):
        assert open(o).read() == "".join("%s @r%d\n" % (tag, k) for k in range(4))
    assert sorted(p.name for p in tmp_path.iterdir()) == ["mea.txt", "pairs.txt", "scan.raw"]


def test_mea_symbol_is_declared_and_exported():
    declared = set(re.findall(r"\b(elemdp_[a-z_0-9]+)\s*\(", open(HEADER).read()))
    assert "elemdp_pair_mea" in declared and "elemdp_pair_mea" in api.SYMBOLS
    assert hasattr(api.load_library(), "elemdp_pair_mea")


def test_pair_weight_is_rounded_before_the_sum():
    """mea_rules.h: a pair candidate is (RN(2 gamma P) + inner) + rest, two roundings where a fused multiply-add would make one.
    At gamma = 1e3 the two differ for most P (at gamma = 0.5, 1, 4 the product is exact and they cannot): the bit-for-bit GPU
    checks at gamma = 1e3 tell a contracted kernel from the rule.  The mirror's score of one pair follows the rule."""
    from fractions import Fraction
    rng = np.random.default_rng(7)
    p, inner = rng.random(200), rng.random(200) * 50.0
    for gamma, differ in ((1e3, True), (0.5, False), (1.0, False), (4.0, False)):
        g2 = 2.0 * gamma
        n = sum((g2 * a + b) != float(Fraction(g2) * Fraction(a) + Fraction(b)) for a, b in zip(p, inner))   # (exact, rounded once)
        assert (n > 20) if differ else (n == 0), (gamma, n)
    L, gamma, pv = 5, 1e3, 0.123456789
    P = np.zeros((L + 1, L + 1))
    kept = np.zeros((L + 1, L + 1), dtype=bool)
    P[0, 5], kept[0, 5] = pv, True
    q = np.full(L, 0.1)
    s, sc = mea_fold(P, kept, q, gamma)
    assert s == "(...)"
    assert sc == ((2.0 * gamma) * pv + ((0.1 + 0.1) + 0.1)) + 0.0
