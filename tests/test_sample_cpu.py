"""Stochastic samples of derivations, host side: the rule of sample_rules.h on the CPU driver's inside
tables against the oracle's posteriors, the generator against its Python mirror, the record format of `scan --out-samples`, the
command line, the sharded writer and the exported symbol."""
import re

import numpy as np
import pytest

from oracle import pyoracle as po
from rnaelem_amd import api, cli, io
from tests.pair_check import oracle_pairs
from tests.sample_check import Driver, check_distribution, check_valid, driver, uniform
from tests.test_host_abi import HEADER
from tests.test_pair_posterior_gpu import PAR, perturbed, ragged_batch

N = 4000


@pytest.mark.parametrize("fast", [False, True])
@pytest.mark.parametrize("pattern", ["((.*.))", "(.....)"])
def test_rule_samples_match_the_oracle_posteriors(pattern, fast):
    seqs, quals = ragged_batch()
    eng = api.Engine(pattern, PAR, 50, 30, 1e-4, 0.1, 0, 0)
    x = perturbed(eng)
    names = eng.describe()["node"]
    M = len(names)
    o = po.make_oracle(pattern, 50, 30, min_bpp=1e-4, tau=0.1)
    o.set_params(x)
    drv = Driver(pattern, PAR)
    drv.set_fast(fast)
    for k, (seq, qual) in enumerate(zip(seqs, quals)):
        rss, nodes, logp, st = drv.sample(x, seq, qual, N, 7, k)
        P = oracle_pairs(o, seq, qual)
        if P is None:
            assert st == 1, k
            continue
        assert st == 0, k
        assert np.all(np.isfinite(logp)) and np.all(logp <= 0.0)
        kept = P > 0.0
        check_valid(rss[:200], nodes[:200], np.ones_like(kept), min(len(seq), 50), M, names, what=(pattern, k))
        check_distribution(rss, nodes, P, o.scan_seq(seq, qual), M, what=(pattern, k))


def test_rule_samples_repeat_and_depend_on_the_key():
    seqs, quals = ragged_batch()
    eng = api.Engine("((.*.))", PAR, 50, 30, 1e-4, 0.1, 0, 0)
    x = perturbed(eng)
    drv = Driver("((.*.))", PAR)
    a = drv.sample(x, seqs[2], quals[2], 50, 3, 2)
    b = drv.sample(x, seqs[2], quals[2], 50, 3, 2)
    assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    assert drv.sample(x, seqs[2], quals[2], 50, 4, 2)[0] != a[0]
    assert drv.sample(x, seqs[2], quals[2], 50, 3, 3)[0] != a[0]
    # the same (rss, nodes) is the same derivation: the same log-probability
    seen = {}
    for r, h, lp in zip(*a[:3]):
        key = (r, h.tobytes())
        if key in seen:
            assert lp == pytest.approx(seen[key], rel=1e-12)
        seen[key] = lp


def test_generator_matches_its_python_mirror():
    keys = [(0, 0, 0, 0), (0, 0, 0, 1), (1, 2, 3, 4), (2 ** 64 - 1, 12345, 99, 7), (42, 10 ** 12, 2 ** 31, 2 ** 40)]
    for key in keys:
        assert driver().emu_sample_uniform(*key) == uniform(*key)
    u = [uniform(5, n, s, d) for n in range(4) for s in range(25) for d in range(40)]
    assert 0.0 <= min(u) and max(u) < 1.0 and abs(np.mean(u) - 0.5) < 0.02


def test_sample_record_formats_and_parses_back(tmp_path):
    names = "z((.*.))o"
    M = len(names)
    rss = ["OLLHRRO", "OOOOOOO"]
    node = np.array([[0, 1, 2, 3, 6, 7, 8], [0, 0, 0, 0, 0, 0, 0]], dtype=np.uint8)
    text = io.sample_record("@r1", (rss, node, np.array([-1.25, -0.5])), names)
    lines = text.split("\n")
    assert lines[:3] == ["id: @r1", "samples: 2", "status: sampled"]
    assert lines[3].split("\t") == ["0", "-1.25", "1", "6", ".((.)).", "OLLHRRO", " ((.)) "]
    assert lines[4].split("\t") == ["1", "-0.5", "-1", "-1", ".......", "OOOOOOO", "       "]
    empty = io.sample_record("@r2", None, names, 2)
    assert empty == "id: @r2\nsamples: 0\nstatus: refused\n"
    path = tmp_path / "s.txt"
    path.write_text(text + empty)
    recs = io.read_sample_records(str(path))
    assert [r[0] for r in recs] == ["@r1", "@r2"]
    assert recs[0][1] == "sampled" and recs[1][1] == "refused"
    assert recs[0][2][0] == (0, -1.25, 1, 6, ".((.)).", "OLLHRRO", " ((.)) ")
    assert recs[0][2][1][2:4] == (-1, -1) and recs[1][2] == []
    assert io.sample_motif_span(node[0], M) == (1, 6)


def test_scan_parser_accepts_the_sample_options():
    a = cli.build_parser().parse_args(["scan", "-f", "x.fq", "-q", "m.txt", "--out1", "a.raw", "--out-samples", "s.txt",
                                       "--n-samples", "7", "--sample-seed", "11"])
    assert a.out_samples == "s.txt" and a.n_samples == 7 and a.sample_seed == 11
    a = cli.build_parser().parse_args(["scan", "-f", "x.fq", "-q", "m.txt", "--out1", "a.raw"])
    assert a.out_samples is None and a.n_samples == 100 and a.sample_seed == 0
    assert "bases" in cli.build_parser()._subparsers._group_actions[0].choices["scan"].format_help()


def test_sharded_writer_joins_the_sample_parts_of_two_ranks_in_input_order(tmp_path):
    recs = [("@r%d" % k, None, None) for k in range(5)]
    out1, outs = str(tmp_path / "scan.raw"), str(tmp_path / "samples.txt")

    def part(mine):
        for rid, _, _ in mine:
            yield "scan %s\n" % rid, "samples %s\n" % rid

    for rank in (1, 0):
        cli.sharded_write(recs, [out1, outs], rank, 2, part, lambda: None)
    assert open(out1).read() == "".join("scan @r%d\n" % k for k in range(5))
    assert open(outs).read() == "".join("samples @r%d\n" % k for k in range(5))
    assert sorted(p.name for p in tmp_path.iterdir()) == ["samples.txt", "scan.raw"]


def test_sample_symbol_is_declared_and_exported():
    declared = set(re.findall(r"\b(elemdp_[a-z_0-9]+)\s*\(", open(HEADER).read()))
    assert "elemdp_sample" in declared and "elemdp_sample" in api.SYMBOLS
    assert hasattr(api.load_library(), "elemdp_sample")
