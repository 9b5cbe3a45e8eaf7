"""Base-pair posteriors under the motif model, host side: the record format of `scan --out-pairs`, the command line, the sharded
writer that joins the per-rank parts, the exported symbols."""
import re

import numpy as np

from rnaelem_amd import api, cli, io
from tests.test_host_abi import HEADER


def test_pair_record_formats_and_parses_back(tmp_path):
    unp = np.array([1.0, 0.25, 0.5, 1.0 - 1e-9, 0.0])
    pairs = (np.array([0, 0, 1], dtype=np.int32), np.array([4, 5, 5], dtype=np.int32), np.array([0.5, 0.25, 0.123456789]))
    text = io.pair_record("@r1", 5, pairs, unp)
    assert text.split("\n")[:6] == ["id: @r1", "unpaired: [1,0.25,0.5,1,0]", "pairs: 3", "1 4 0.5", "1 5 0.25", "2 5 0.123457"]
    empty = io.pair_record("@r2", 3, (np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0)), np.ones(3))
    assert empty == "id: @r2\nunpaired: [1,1,1]\npairs: 0\n"
    path = tmp_path / "p.txt"
    path.write_text(text + empty)
    recs = io.read_pair_records(str(path))
    assert [r[0] for r in recs] == ["@r1", "@r2"]
    np.testing.assert_allclose(recs[0][1], unp, rtol=1e-6)
    assert recs[0][2] == [(1, 4, 0.5), (1, 5, 0.25), (2, 5, 0.123457)]
    assert list(recs[1][1]) == [1.0, 1.0, 1.0] and recs[1][2] == []


def test_scan_parser_accepts_the_pair_options():
    a = cli.build_parser().parse_args(["scan", "-f", "x.fq", "-q", "m.txt", "--out1", "a.raw", "--out-pairs", "p.txt",
                                       "--pair-min-prob", "0.01"])
    assert a.out_pairs == "p.txt" and a.pair_min_prob == 0.01
    a = cli.build_parser().parse_args(["scan", "-f", "x.fq", "-q", "m.txt", "--out1", "a.raw"])
    assert a.out_pairs is None and a.pair_min_prob == 1e-3


def test_sharded_writer_joins_the_pair_parts_of_two_ranks_in_input_order(tmp_path):
    recs = [("@r%d" % k, None, None) for k in range(5)]
    out1, outp = str(tmp_path / "scan.raw"), str(tmp_path / "pairs.txt")

    def part(mine):
        for rid, _, _ in mine:
            yield "scan %s\n" % rid, "pairs %s\n" % rid

    for rank in (1, 0):     # (rank 0 joins after the other rank's parts exist; the barrier has nothing to wait for)
        cli.sharded_scan(recs, out1, rank, 2, part, lambda: None, out_pairs=outp)
    assert open(out1).read() == "".join("scan @r%d\n" % k for k in range(5))
    assert open(outp).read() == "".join("pairs @r%d\n" % k for k in range(5))
    assert sorted(p.name for p in tmp_path.iterdir()) == ["pairs.txt", "scan.raw"]
    # the call of today (no pair file) is unchanged: the texts alone
    cli.sharded_scan(recs, out1, 0, 1, lambda mine: ("s %s\n" % r[0] for r in mine), lambda: None)
    assert open(out1).read() == "".join("s @r%d\n" % k for k in range(5))


def test_pair_symbols_are_declared_and_exported():
    declared = set(re.findall(r"\b(elemdp_[a-z_0-9]+)\s*\(", open(HEADER).read()))
    for name in ("elemdp_pair_posteriors", "elemdp_pair_list"):
        assert name in declared and name in api.SYMBOLS
        assert hasattr(api.load_library(), name)
