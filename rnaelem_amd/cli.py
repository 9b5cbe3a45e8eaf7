"""Command line of the path: the option names of the reference binary's `train` / `scan` sub-commands
(RNAelem/application.hpp option table; what `script/elem` spawns), driving libelemdp instead of the CPU DP.

    python -m rnaelem_amd.cli train --fastq pos.fq --motif-pattern '((.*.))' --out1 model.txt --no-shuffle [-i 300]
    python -m rnaelem_amd.cli scan  --fastq seqs.fq --motif-model model.txt --out1 scan.raw
    python -m rnaelem_amd.cli scan  --fastq seqs.fq --motif-model model.txt --out1 scan.raw --out-pairs pairs.txt
                                    # + base-pair posteriors under the motif model (--pair-min-prob, default 1e-3)
    python -m rnaelem_amd.cli scan  --fastq seqs.fq --motif-model model.txt --out1 scan.raw --out-mea mea.txt
                                    # + maximum expected accuracy structures over those posteriors (--mea-gamma, default 1)
    python -m rnaelem_amd.cli scan  --fastq seqs.fq --motif-model model.txt --out1 scan.raw --out-samples samples.txt
                                    # + sampled structures with their motif alignments (--n-samples 100, --sample-seed 0)
    python -m rnaelem_amd.cli scan  --fastq seqs.fq --motif-model model.txt --out1 scan.raw --out-context ctx.txt
                                    # + structural context profiles: P(O L R H B I M) of every base (io.context_record)
    python -m rnaelem_amd.cli scan  --fastq seqs.fq --motif-model model.txt --out1 scan.raw --out-nodes nodes.txt
                                    # + posterior motif-node profiles: P(node) of every base and the confidence of the printed
                                    #   alignment (io.node_record)
    python -m rnaelem_amd.cli scan  --fastq seqs.fq --motif-model model.txt --out1 scan.raw --out-sites sites.txt
                                    # + maximum expected accuracy motif alignments and site lists decoded from those profiles
                                    #   (--site-gamma 1.0, --max-sites 1; io.site_record)
    python -m rnaelem_amd.cli scan  --fastq seqs.fq --motif-model model.txt --out1 scan.raw --out-contrast contrast.txt
                                    # + the fold with the motif against the fold without it: pair posteriors, unpaired and
                                    #   MEA structure of each (--contrast-min-prob 1e-3, --contrast-gamma 1.0; io.contrast_record)
    python -m rnaelem_amd.cli scan  --fastq seqs.fq --motif-model model.txt --out1 scan.raw --out-access access.txt
                                    # + accessibility: the probability that the window of width 1 .. --access-width (16) at
                                    #   every base is unpaired (io.access_record)
    python -m rnaelem_amd.cli scan  --fastq seqs.fq --motif-model model.txt --out1 scan.raw --out-logo logo.txt
                                    # + the table behind a motif logo: per pattern node the expected emission counts of each base
                                    #   under each structure letter, over the sequences with exist_prob >= --logo-min-exist (0)
                                    #   (io.write_logo)
    python -m rnaelem_amd.cli scan  --fastq seqs.fq --motif-model model.txt --out1 scan.raw --out-stems stems.txt --out-stem-pairs sp.txt
                                    # + the table behind a stem logo: per pair of pattern nodes that emit a base pair jointly the
                                    #   expected counts of each left and right base, over the sequences with exist_prob >=
                                    #   --logo-min-exist (io.write_stems); and one line per base pair and node pair with
                                    #   probability >= --stem-min-prob (0.01) (io.stem_pair_line)
    python -m rnaelem_amd.cli scan  --fastq seqs.fq --motif-model model.txt --out1 scan.raw --out-pairs pairs.txt --constraints cons.txt
                                    # every result under hard structure constraints per sequence: '>id', then one character
                                    #   per base, . x | < > ( ) (also `eval --constraints`; io.read_constraints)
    python -m rnaelem_amd.cli       --fastq pos.fq --motif-pattern '((.*.))' --out1 model.txt --out2 scan.raw
                                    # no sub-command = what script/elem spawns: train, write the model, scan (main.cpp:47-84)
    python -m rnaelem_amd.cli eval  --fastq pos.fq --motif-model model.txt --out1 fn.txt --out2 gr.txt     (motif_eval.hpp:23-54)
    python -m rnaelem_amd.cli array-eval --array N --task-id K ... --out4 part   # part K of N: index / range / fn / gr / sum eff
    torchrun --nproc-per-node 8 -m rnaelem_amd.cli train ...      # one rank per GPU, one RCCL all-reduce per evaluation
    torchrun --nproc-per-node 8 -m rnaelem_amd.cli scan ...       # ranks scan contiguous ranges; rank 0 joins them in input order

Implemented: full-batch training -- `--no-shuffle` (L-BFGS-B, the path named by BASELINE.json) and the default mode with
per-iteration shuffled negatives (Adam, `--kmer-shuf`) --, mini-batches (`--batch-size N`), all of them on one or several
GPUs (torchrun), `--lik-ratio`,
`--param-set`, `--theta-softmax`, and `scan`.  Not implemented: grid-engine array jobs (out of scope).
"""
import argparse
import os
import sys

import numpy as np

from . import api, io, train as trainer
from .distributed import ShardedPairs, ShardedShuffledNegatives, ShardedTrainer


def build_parser():
    p = argparse.ArgumentParser(prog="rnaelem_amd.cli", description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = p.add_subparsers(dest="cmd", required=True)
    for name in ("train", "scan", "normal", "eval", "array-eval"):
        s = sub.add_parser(name)
        s.add_argument("-f", "--fastq", required=True, help="input FASTQ with pseudo-qualities (L+1 quality characters)")
        s.add_argument("--out1", required=name != "array-eval", help="train / normal: model file; scan: raw records; eval: 'fn:' line")
        s.add_argument("--device", type=int, default=None, help="GPU index (default: LOCAL_RANK or 0)")
    for name in ("train", "normal"):
        _train_options(sub.choices[name])
    sub.choices["normal"].add_argument("--out2", required=True, help="raw scan records of the training sequences")
    for name in ("scan", "eval", "array-eval"):
        sub.choices[name].add_argument("-q", "--motif-model", required=True)
    for name in ("scan", "normal"):
        sub.choices[name].add_argument("--chunk", type=int, default=20000,
                                       help="sequences resident on the GPU at a time (plan + tables; BASELINE config E = 100 k x L=300 "
                                            "does not fit at once)")
    sub.choices["scan"].add_argument("--out-pairs", default=None,
                                     help="base-pair posteriors under the motif model: one record per sequence (io.pair_record)")
    sub.choices["scan"].add_argument("--pair-min-prob", type=float, default=1e-3, help="pairs below this probability are left out")
    sub.choices["scan"].add_argument("--out-mea", default=None,
                                     help="maximum expected accuracy structures under the motif model: one record per sequence "
                                          "(io.mea_record)")
    sub.choices["scan"].add_argument("--mea-gamma", type=float, default=1.0,
                                     help="weight of the pairs: a pair scores 2 gamma P, an unpaired base its unpaired probability")
    sub.choices["scan"].add_argument("--out-samples", default=None,
                                     help="stochastic samples of structures with their motif alignments: one record per sequence "
                                          "(io.sample_record).  Host memory per chunk: n-samples x bases of the chunk x 2 bytes")
    sub.choices["scan"].add_argument("--n-samples", type=int, default=100, help="samples per sequence")
    sub.choices["scan"].add_argument("--sample-seed", type=int, default=0,
                                     help="seed of the draws (with the sequence's input index: a torchrun run writes what one GPU writes)")
    sub.choices["scan"].add_argument("--out-context", default=None,
                                     help="structural context profiles under the motif model: one record per sequence "
                                          "(io.context_record)")
    sub.choices["scan"].add_argument("--out-nodes", default=None,
                                     help="posterior motif-node profiles under the motif model: one record per sequence "
                                          "(io.node_record), with the confidence of the psihat line of --out1")
    sub.choices["scan"].add_argument("--out-sites", default=None,
                                     help="maximum expected accuracy motif alignments and site lists decoded from the node "
                                          "profile: one record per sequence (io.site_record)")
    sub.choices["scan"].add_argument("--site-gamma", type=float, default=1.0,
                                     help="weight of the pattern's nodes: a base on a pattern node scores gamma N, on z or o its N")
    sub.choices["scan"].add_argument("--max-sites", type=int, default=1, help="most sites reported per sequence (1 .. 64)")
    sub.choices["scan"].add_argument("--out-contrast", default=None,
                                     help="motif-conditional pair posteriors, the fold with the motif against the fold without it: "
                                          "one record per sequence (io.contrast_record)")
    sub.choices["scan"].add_argument("--contrast-min-prob", type=float, default=1e-3,
                                     help="pairs below this probability in both folds are left out")
    sub.choices["scan"].add_argument("--contrast-gamma", type=float, default=1.0, help="weight of the pairs in the two structures (as --mea-gamma)")
    sub.choices["scan"].add_argument("--out-access", default=None,
                                     help="accessibility under the motif model, the probability that a window of bases is unpaired: "
                                          "one record per sequence (io.access_record)")
    sub.choices["scan"].add_argument("--access-width", type=int, default=16, help="widest window (1 .. 64)")
    sub.choices["scan"].add_argument("--out-logo", default=None,
                                     help="the table behind a motif logo: per pattern node the expected emission counts of each base "
                                          "under each structure letter, summed over the sequences (io.write_logo)")
    sub.choices["scan"].add_argument("--logo-min-exist", type=float, default=0.0,
                                     help="only sequences whose exist_prob is at least this enter the logo table")
    sub.choices["scan"].add_argument("--out-stems", default=None,
                                     help="the table behind a stem logo: per pair of pattern nodes that emit a base pair jointly the "
                                          "expected counts of each left and right base, summed over the sequences that pass "
                                          "--logo-min-exist (io.write_stems)")
    sub.choices["scan"].add_argument("--out-stem-pairs", default=None,
                                     help="base pairs labelled by the pair of pattern nodes that emits them: one line per entry with "
                                          "sequence id, i, j, the two nodes and the probability (io.stem_pair_line)")
    sub.choices["scan"].add_argument("--stem-min-prob", type=float, default=0.01, help="smallest probability listed in --out-stem-pairs")
    sub.choices["scan"].add_argument("--out-helices", default=None,
                                     help="helix posteriors, the joint probability that a run of directly stacked pairs forms: one line "
                                          "per entry with sequence id, i, j of the outermost pair (as --out-stem-pairs), the number of "
                                          "pairs and the probability (io.helix_line)")
    sub.choices["scan"].add_argument("--helix-min-prob", type=float, default=0.01, help="smallest probability listed in --out-helices")
    sub.choices["scan"].add_argument("--helix-min-len", type=int, default=2, help="shortest helix listed in --out-helices")
    sub.choices["scan"].add_argument("--helix-max-len", type=int, default=16, help="longest helix listed in --out-helices (1 .. 32)")
    sub.choices["scan"].add_argument("--out-mea-helices", default=None,
                                     help="the stems of the maximum expected accuracy structure at --mea-gamma: one line per stem with "
                                          "sequence id, i, j, length, the joint probability of the whole stem and the smallest pair "
                                          "posterior in it (io.mea_helix_line); costs one MEA call (shared with --out-mea) and one "
                                          "helix call (shared with --out-helices)")
    sub.choices["scan"].add_argument("--out-loops", default=None,
                                     help="loop posteriors, what every listed pair closes: one line per entry with sequence id, type "
                                          "letter (H S B I M), i, j of the closing pair (as --out-helices), k, l of the inner pair of "
                                          "a bulge or an interior loop (- - otherwise) and the probability (io.loop_line)")
    sub.choices["scan"].add_argument("--loop-min-prob", type=float, default=0.01, help="smallest pair posterior and two-loop probability listed in --out-loops")
    sub.choices["scan"].add_argument("--out-mea-loops", default=None,
                                     help="the loops of the maximum expected accuracy structure at --mea-gamma: one line per pair with "
                                          "the fields of --out-loops for the loop it closes, then the pair posterior of the closing pair "
                                          "(io.mea_loop_line); costs one MEA call (shared with --out-mea) and one loop call (shared "
                                          "with --out-loops)")
    sub.choices["scan"].add_argument("--world", choices=list(api.WORLDS), default="mixed",
                                     help="the ensemble every --out-* product but --out-contrast describes: the mixture of the parses "
                                          "with the motif and those without it (mixed), the parses with the motif alone (motif) or "
                                          "those without it alone (none); --out1 is the same in every world.  A product file of a "
                                          "world other than mixed starts with the line '# world: <world>'")
    for name in ("scan", "eval"):
        sub.choices[name].add_argument("--constraints", default=None, metavar="FILE",
                                       help="hard structure constraints (DESIGN.md section 26): a FASTA-like file, '>id' of a FASTQ "
                                            "record, then one character per base: . free, x unpaired, | paired, < > paired as the 5' / 3' "
                                            "base, ( ) these two bases pair.  Records the file does not name are free; an id the FASTQ "
                                            "lacks or a string of another length than its sequence ends the run.  Every result then "
                                            "describes the constrained ensemble, and a product file starts with the line "
                                            "'# constraints: <file>'.  (train takes no constraints: its shuffled negatives and "
                                            "look-ahead loads would need a policy of their own.)")
    sub.choices["eval"].add_argument("--out2", required=True, help="'gr:' line")
    a = sub.choices["array-eval"]
    a.add_argument("-a", "--array", type=int, required=True, help="number of parts")
    a.add_argument("--task-id", type=int, default=None, help="1-based part (default: $SGE_TASK_ID)")
    a.add_argument("--out4", required=True, help="result file prefix: <out4>-<task id> (motif_array_trainer.hpp:25)")
    for name in ("eval", "array-eval"):
        sub.choices[name].add_argument("--lik-ratio", action="store_true")
    return p


def _train_options(t):
    t.add_argument("-m", "--motif-pattern", required=True)
    t.add_argument("-i", "--max-iter", type=int, default=300)
    t.add_argument("--energy-param", default="~T2004~")
    t.add_argument("-w", "--max-span", type=int, default=50)
    t.add_argument("-c", "--max-internal-loop", type=int, default=30)
    t.add_argument("--epsilon", type=float, default=1e-3)
    t.add_argument("--rho-s", type=float, default=0.1)
    t.add_argument("--rho-theta", type=float, default=0.1)
    t.add_argument("--rho-lambda", type=float, default=0.1)
    t.add_argument("--tau", type=float, default=0.1)
    t.add_argument("--lambda-init", type=float, default=0.0)
    t.add_argument("--lambda-prior", type=float, default=0.0)
    t.add_argument("-p", "--min-bpp", type=float, default=1e-4)
    t.add_argument("--no-rss", action="store_true")
    t.add_argument("--no-profile", action="store_true")
    t.add_argument("--no-energy", action="store_true")
    t.add_argument("--no-shuffle", action="store_true")
    t.add_argument("--theta-softmax", action="store_true")
    t.add_argument("--lik-ratio", action="store_true")
    t.add_argument("--batch-size", type=int, default=-1)
    t.add_argument("--kmer-shuf", type=int, default=2)
    t.add_argument("--param-set", default=None, help="comma separated indexes of the parameters to fit (the others stay fixed)")
    t.add_argument("--optimizer", choices=["lbfgsb", "adam"], default="lbfgsb")


def parse_param_set(spec):
    """--param-set: comma separated indexes or ranges `a-b` (inclusive), as application.hpp:376-388 reads it"""
    out = []
    for part in spec.split(","):
        se = [int(v) for v in part.split("-")]
        out += [se[0]] if len(se) == 1 else list(range(se[0], se[1] + 1))
    return out


def _rank_world():
    return int(os.environ.get("RANK", "0")), int(os.environ.get("LOCAL_RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))


def cmd_train(a):
    rank, local_rank, world = _rank_world()
    if world > 1:
        import torch
        import torch.distributed as dist
        torch.cuda.set_device(local_rank)
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("nccl", rank=rank, world_size=world)
    flags = (api.NO_RSS if a.no_rss else 0) | (api.NO_PROFILE if a.no_profile else 0) | (api.NO_ENERGY if a.no_energy else 0) | \
        (api.THETA_SOFTMAX if a.theta_softmax else 0) | (api.LIK_RATIO if a.lik_ratio else 0)
    pattern = a.motif_pattern.replace("_", ".") if a.no_rss else a.motif_pattern
    par = a.energy_param if a.energy_param in ("~T2004~", "~A2007~") else open(a.energy_param).read()
    device = a.device if a.device is not None else local_rank
    eng = api.Engine(pattern, par, a.max_span, a.max_internal_loop, a.min_bpp, a.tau, flags, device)
    recs = io.read_fastq(a.fastq)
    seqs, quals = [s for _, s, _ in recs], [q for _, _, q in recs]
    sharded_pairs = world > 1 and (not a.no_shuffle or a.batch_size > 0)
    ev = None if (a.batch_size > 0 or sharded_pairs) else ShardedTrainer(eng, seqs, quals, rank, world)
    x0 = eng.initial_params(a.lambda_init)
    log = (lambda msg: print(msg, file=sys.stderr, flush=True)) if rank == 0 else None
    vary = parse_param_set(a.param_set) if a.param_set else None
    optimizer = a.optimizer
    if sharded_pairs:      # several GPUs: records (and their negatives) sharded per evaluation, one all-reduce
        neg = api.Engine(pattern, par, a.max_span, a.max_internal_loop, a.min_bpp, a.tau, flags, device)
        pairs = ShardedPairs.on_engines(eng, neg, rank, world, None if a.no_shuffle else a.kmer_shuf)
        if a.batch_size > 0:
            ev = trainer.MiniBatches(seqs, quals, a.batch_size, None, pairs=pairs)
        else:
            ev = ShardedShuffledNegatives(pairs, seqs, quals)
        optimizer = "lbfgsb" if a.no_shuffle else "adam"
    elif a.batch_size > 0:   # mini-batches: every evaluation loads the next records of the epoch order (motif_trainer.hpp:595-632)
        def eval_batch(s2, q2, x):
            eng.load_batch(s2, q2)
            return eng.train_eval(x) + (eng.seq_stats()[:, 4] != 0,)

        eng2 = api.Engine(pattern, par, a.max_span, a.max_internal_loop, a.min_bpp, a.tau, flags, device)
        # (double-buffered: the next batch loads on one engine while the other evaluates the current one)
        ev = trainer.MiniBatches(seqs, quals, a.batch_size, eval_batch, None if a.no_shuffle else a.kmer_shuf, engines=[eng, eng2])
        optimizer = "lbfgsb" if a.no_shuffle else "adam"
    elif not a.no_shuffle:   # default `elem train`: Adam over positives + per-iteration shuffled negatives (main.cpp:132-152)
        neg = api.Engine(pattern, par, a.max_span, a.max_internal_loop, a.min_bpp, a.tau, flags, device)

        def eval_neg(s2, q2, x):
            neg.load_batch(s2, q2)
            return neg.train_eval(x)

        ev = trainer.ShuffledNegatives(seqs, eng.train_eval, lambda: eng.seq_stats()[:, 4] != 0, eval_neg, a.kmer_shuf)
        optimizer = "adam"
    res = trainer.train(ev, x0, a.rho_s if a.theta_softmax else a.rho_theta, a.rho_lambda, a.max_iter, a.epsilon, optimizer, log, vary)
    if hasattr(ev, "finish"):
        ev.finish()
    if rank == 0:
        d = eng.describe()
        rows, k = [], 0
        for w in d["theta_sizes"]:
            rows.append([0.0] * w)
            k += w
        m = dict(pattern=pattern, rows=rows, lam=[0.0, 0.0], softmax=a.theta_softmax, ene_param=a.energy_param, max_span=a.max_span,
                 max_iloop=a.max_internal_loop, min_bpp=a.min_bpp, tau=a.tau, rho_theta=a.rho_theta, rho_s=a.rho_s,
                 rho_lambda=a.rho_lambda, lambda_prior=a.lambda_prior, no_rss=a.no_rss, no_prf=a.no_profile, no_ene=a.no_energy)
        io.write_model(a.out1, m, res["x"])
        print("%s after %d iterations (%d evaluations); final value: %.6g" % (res["message"], res["n_iter"], res["n_eval"], res["f"]),
              file=sys.stderr)
    if a.cmd == "normal":     # main.cpp:73-81: the trained model scans the training sequences
        m = io.read_model(a.out1) if rank == 0 else None
        if world > 1:
            box = [m]
            dist.broadcast_object_list(box, src=0)
            m = box[0]
        _scan_records(eng, m, recs, a.out2, a.chunk, rank, world, (lambda: dist.barrier()) if world > 1 else (lambda: None))
    if world > 1:
        dist.destroy_process_group()


def world_header(scan_world):
    """The first line of a product file written in a world other than the mixture ('' for the mixture)."""
    return "" if scan_world == "mixed" else "# world: %s\n" % scan_world


def constraints_header(path):
    """The line a product file written under --constraints starts with ('' without)."""
    return "" if path is None else "# constraints: %s\n" % path


def read_constraints_for(recs, path):
    """The constraint of every record (io.constraints_for) from the file of --constraints, None without one; a file the records do
    not fit ends the run with the message."""
    if path is None:
        return None
    try:
        return io.constraints_for(recs, io.read_constraints(path), path)
    except ValueError as e:
        raise SystemExit("--constraints: %s" % e)


def sharded_write(recs, outs, rank, world, part, barrier, headers=None):
    """Rank k handles the contiguous range assigned_range(n, world, k): `part(records)` yields one tuple of texts per record, one
    text per file of `outs`, written to `<out>.<k>`; after a barrier rank 0 joins the parts of every file in rank order = input
    order.  headers: one text per file of `outs` that the joined file starts with (none by default)."""
    from .distributed import assigned_range
    lo, hi = assigned_range(len(recs), world, rank)
    names = list(outs) if world == 1 else ["%s.%d" % (o, rank) for o in outs]
    headers = list(headers) if headers is not None else [""] * len(outs)
    files = [open(nm, "w") for nm in names]
    try:
        if world == 1:
            for f, h in zip(files, headers):
                f.write(h)
        for texts in part(recs[lo:hi]):
            for f, t in zip(files, texts):
                f.write(t)
    finally:
        for f in files:
            f.close()
    if world == 1:
        return
    barrier()
    if rank == 0:
        for o, h in zip(outs, headers):
            with open(o, "w") as f:
                f.write(h)
                for k in range(world):
                    name = "%s.%d" % (o, k)
                    with open(name) as g:
                        for line in g:
                            f.write(line)
                    os.remove(name)
    barrier()


def sharded_scan(recs, out1, rank, world, scan_part, barrier, out_pairs=None, pairs_header=""):
    """Scan needs no collective: rank k scans the contiguous range assigned_range(n, world, k) and writes
    `<out1>.<k>`; after a barrier rank 0 joins the parts in rank order = input order into `out1` (the reference's writer
    emits records as its threads finish, motif_scanner.hpp:237-252; here the order is the input's).  `scan_part(records)`
    yields the record texts of a list of (id, codes, quals); with `out_pairs` it yields (scan record, pair record) tuples and
    the pair records are joined into `out_pairs` the same way."""
    if out_pairs is None:
        sharded_write(recs, [out1], rank, world, lambda mine: ((t,) for t in scan_part(mine)), barrier)
    else:
        sharded_write(recs, [out1, out_pairs], rank, world, scan_part, barrier, ["", pairs_header])


def _scan_records(eng, m, recs, out1, chunk, rank, world, barrier, out_pairs=None, pair_min_prob=1e-3, out_mea=None, mea_gamma=1.0,
                  out_samples=None, n_samples=100, sample_seed=0, out_context=None, out_nodes=None, out_sites=None, site_gamma=1.0,
                  max_sites=1, out_contrast=None, contrast_min_prob=1e-3, contrast_gamma=1.0, out_access=None, access_width=16, out_logo=None,
                  logo_min_exist=0.0, out_stems=None, out_stem_pairs=None, stem_min_prob=0.01, out_helices=None, helix_min_prob=0.01,
                  helix_min_len=2, helix_max_len=16, out_mea_helices=None, out_loops=None, loop_min_prob=0.01, out_mea_loops=None,
                  scan_world="mixed", constraints=None, constraints_path=None):
    """constraints: a hard structure constraint per record of `recs` (None entries free), or None; a product file then starts
    with constraints_header(constraints_path).  scan_world: the world ("mixed", "motif", "none"; Engine option world) of every product but the contrast file, which holds
    both worlds; the scan records are the same in every world.  A product file of a world other than mixed starts with
    world_header(scan_world)."""
    from .distributed import assigned_range
    sw = dict(world=scan_world)
    head = constraints_header(constraints_path if constraints is not None else None) + world_header(scan_world)
    stem_parts = None if out_stems is None else out_stems + ".seqs"   # (as logo_parts)
    want_stems = out_stems is not None or out_stem_pairs is not None
    want_helices = out_helices is not None or out_mea_helices is not None
    want_loops = out_loops is not None or out_mea_loops is not None
    want_every = out_mea_helices is not None or out_mea_loops is not None   # (the MEA call lists every pair)
    slots = eng.stem_slots() if want_stems else None                  # (the model's: once per run)
    logo_parts = None if out_logo is None else out_logo + ".seqs"     # (per-sequence counts, joined in input order before the sum)
    nodes = eng.describe()["node"]
    step = max(1, chunk)
    lo = assigned_range(len(recs), world, rank)[0]     # (batch-global sequence index of this rank's first record: the samples' key)

    def scan_part(mine):
        for c0 in range(0, len(mine), step):        # records are independent: chunks in input order
            part = mine[c0:c0 + step]
            if constraints is None:
                eng.load_batch([s for _, s, _ in part], [q for _, _, q in part])
            else:   # (the strings of this rank's records, chunk by chunk)
                eng.load_batch([s for _, s, _ in part], [q for _, _, q in part], constraints=constraints[lo + c0:lo + c0 + len(part)])
            res, en = eng.scan(m["x"])
            if out_pairs is None and out_mea is None and out_samples is None and out_context is None and out_nodes is None and out_sites is None \
                    and out_contrast is None and out_access is None and out_logo is None and not want_stems and not want_helices \
                    and not want_loops:
                for (rid, codes, _), r in zip(part, res):
                    yield io.scan_record(rid, codes, r, nodes)
                continue
            # (the same loaded batch; with both files one device call gives the pairs and the structures)
            if out_mea is None and not want_every:
                prs = eng.pair_posteriors(m["x"], pair_min_prob, **sw) if out_pairs is not None else None
            elif not want_every:
                structs, scores, prs = eng.mea_structures(m["x"], mea_gamma, pair_min_prob if out_pairs is not None else None, **sw)
            else:   # (the stems' smallest pair posterior comes from this call's own list: every pair, cut to --pair-min-prob for the pairs file)
                structs, scores, every = eng.mea_structures(m["x"], mea_gamma, 0.0, **sw)
                prs = [(ii[pp >= pair_min_prob], jj[pp >= pair_min_prob], pp[pp >= pair_min_prob], unp) for ii, jj, pp, unp in every]
            smp = eng.sample_structures(m["x"], n_samples, sample_seed, lo + c0, **sw) if out_samples is not None else None
            ctx = eng.context_profiles(m["x"], **sw) if out_context is not None else None
            # (with both files one node pass gives the profiles and the sites)
            if out_sites is not None:
                sit = eng.mea_alignments(m["x"], site_gamma, max_sites, profile=out_nodes is not None, **sw)
                nod = [r["profile"] for r in sit] if out_nodes is not None else None
            else:
                nod = eng.node_profiles(m["x"], **sw) if out_nodes is not None else None
            con = eng.conditional_pairs(m["x"], contrast_min_prob, contrast_gamma) if out_contrast is not None else None
            acc = eng.accessibility(m["x"], access_width, **sw) if out_access is not None else None
            jnt = eng.joint_profiles(m["x"], **sw) if out_logo is not None else None
            if want_stems:      # (one call gives the counts and the list)
                stm = eng.stem_profiles(m["x"], stem_min_prob if out_stem_pairs is not None else np.inf, **sw)
                stm_counts, stm_lists = stm if out_stem_pairs is not None else (stm, None)
            if want_helices:    # (one call gives the list and the stems of the MEA structures)
                hlx = eng.helix_posteriors(m["x"], helix_min_prob if out_helices is not None else np.inf, helix_min_len, helix_max_len,
                                           structs if out_mea_helices is not None else None, **sw)
                hlx_lists, hlx_stems = hlx if out_mea_helices is not None else (hlx, None)
            if want_loops:      # (one call gives the lists and the loops of the MEA structures)
                lps = eng.loop_posteriors(m["x"], loop_min_prob if out_loops is not None else np.inf,
                                          structs if out_mea_loops is not None else None, counts=False, **sw)
                lp_closing, lp_two = lps[0], lps[1]
                lp_mea = lps[3] if out_mea_loops is not None else None
            for k, ((rid, codes, _), r) in enumerate(zip(part, res)):
                texts = [io.scan_record(rid, codes, r, nodes)]
                if out_pairs is not None:
                    ii, jj, pp, unp = prs[k]
                    texts.append(io.pair_record(rid, len(codes), (ii, jj, pp), unp))
                if out_mea is not None:
                    texts.append(io.mea_record(rid, structs[k], scores[k]))
                if out_samples is not None:
                    rss, node, logp, status = smp[k]
                    texts.append(io.sample_record(rid, (rss, node, logp) if status == eng.SAMPLED else None, nodes, status))
                if out_context is not None:
                    texts.append(io.context_record(rid, ctx[k]))
                if out_nodes is not None:
                    texts.append(io.node_record(rid, nod[k], nodes, api.alignment_confidence(nod[k], r["psihat"])))
                if out_sites is not None:
                    texts.append(io.site_record(rid, sit[k], nodes))
                if out_contrast is not None:
                    texts.append(io.contrast_record(rid, con[k]))
                if out_access is not None:
                    texts.append(io.access_record(rid, acc[k]))
                if out_logo is not None:
                    texts.append(io.logo_counts_record(rid, r["exist_prob"], jnt[k]))
                if out_stem_pairs is not None:
                    texts.append("".join(io.stem_pair_line(rid, i + 1, j, "%d%s" % (slots[t, 0], nodes[slots[t, 0]]),
                                                           "%d%s" % (slots[t, 1], nodes[slots[t, 1]]), q) for i, j, t, q in zip(*stm_lists[k])))
                if out_stems is not None:
                    texts.append(io.stem_counts_record(rid, r["exist_prob"], stm_counts[k]))
                if out_helices is not None:
                    texts.append("".join(io.helix_line(rid, i + 1, j, n, p) for i, j, n, p in zip(*hlx_lists[k])))
                if out_mea_helices is not None:
                    texts.append("".join(io.mea_helix_line(rid, i + 1, j, n, p, api.stem_min_posterior(every[k], i, j, n))
                                         for i, j, n, p in zip(*hlx_stems[k])))
                if out_loops is not None:
                    texts.append(io.loop_lines(rid, lp_closing[k], lp_two[k]))
                if out_mea_loops is not None:
                    have = {(int(a), int(b)): float(v) for a, b, v in zip(every[k][0], every[k][1], every[k][2])}
                    texts.append("".join(io.mea_loop_line(rid, api.LOOP_TYPES[t], i + 1, j, kk + 1 if kk >= 0 else None, ll, p,
                                                          have.get((int(i), int(j)), 0.0)) for t, i, j, kk, ll, p in zip(*lp_mea[k])))
                yield tuple(texts)

    if out_mea is None and out_samples is None and out_context is None and out_nodes is None and out_sites is None and out_contrast is None \
            and out_access is None and out_logo is None and not want_stems and not want_helices and not want_loops:
        sharded_scan(recs, out1, rank, world, scan_part, barrier, out_pairs, head)
    else:
        outs = [out1] + [o for o in (out_pairs, out_mea, out_samples, out_context, out_nodes, out_sites, out_contrast, out_access, logo_parts,
                                   out_stem_pairs, stem_parts, out_helices, out_mea_helices, out_loops, out_mea_loops) if o is not None]
        # (no header on the scan records, the contrast file and the per-sequence records the two tables are summed from)
        plain = (out1, out_contrast, logo_parts, stem_parts)
        sharded_write(recs, outs, rank, world, scan_part, barrier, ["" if o in plain else head for o in outs])
    if out_logo is not None:
        if rank == 0:
            write_logo_from_parts(logo_parts, out_logo, nodes, logo_min_exist)
            _prepend(out_logo, head)
        barrier()
    if out_stems is not None:
        if rank == 0:
            write_stems_from_parts(stem_parts, out_stems, nodes, slots, logo_min_exist)
            _prepend(out_stems, head)
        barrier()


def _prepend(path, head):
    """Put `head` in front of a (small) finished file; nothing to do for an empty head."""
    if not head:
        return
    with open(path) as f:
        body = f.read()
    with open(path, "w") as f:
        f.write(head + body)


def write_stems_from_parts(parts_path, out_stems, nodes, slots, min_exist=0.0):
    """The `--out-stems` file from the per-sequence count records in input order: the sequences with exist_prob >= min_exist are
    summed in that order (api.stem_logo with weights 1 / 0); the records file is removed."""
    parts = io.read_stem_counts(parts_path)
    use = np.array([1.0 if ex >= min_exist else 0.0 for _, ex, _ in parts])
    counts = np.stack([c for _, _, c in parts]) if parts else np.zeros((0, len(slots), 5, 5))
    io.write_stems(out_stems, nodes, slots, api.stem_logo(counts, slots, nodes, use)["counts"], int(use.sum()), len(parts))
    os.remove(parts_path)


def write_logo_from_parts(parts_path, out_logo, nodes, min_exist=0.0):
    """The `--out-logo` file from the per-sequence count records in input order: the sequences with exist_prob >= min_exist are
    summed in that order (api.motif_logo with weights 1 / 0); the records file is removed."""
    parts = io.read_logo_counts(parts_path)
    use = np.array([1.0 if ex >= min_exist else 0.0 for _, ex, _ in parts])
    counts = np.stack([c for _, _, c in parts]) if parts else np.zeros((0, len(nodes), 7, 5))
    io.write_logo(out_logo, nodes, api.motif_logo(counts, use)["counts"], int(use.sum()), len(parts))
    os.remove(parts_path)


def cmd_scan(a):
    rank, local_rank, world = _rank_world()
    barrier = lambda: None
    if world > 1:     # only for the barrier around the join of the per-rank files: gloo, no device collective
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("gloo", rank=rank, world_size=world)
        barrier = dist.barrier
    m = io.read_model(a.motif_model)
    eng = io.engine_from_model(m, a.device if a.device is not None else local_rank)
    recs = io.read_fastq(a.fastq)
    _scan_records(eng, m, recs, a.out1, a.chunk, rank, world, barrier, a.out_pairs, a.pair_min_prob, a.out_mea,
                  a.mea_gamma, a.out_samples, a.n_samples, a.sample_seed, a.out_context, a.out_nodes, a.out_sites, a.site_gamma, a.max_sites,
                  a.out_contrast, a.contrast_min_prob, a.contrast_gamma, a.out_access, a.access_width, a.out_logo, a.logo_min_exist,
                  a.out_stems, a.out_stem_pairs, a.stem_min_prob, a.out_helices, a.helix_min_prob, a.helix_min_len, a.helix_max_len,
                  a.out_mea_helices, a.out_loops, a.loop_min_prob, a.out_mea_loops, a.world,
                  read_constraints_for(recs, a.constraints), a.constraints)
    if world > 1:
        dist.destroy_process_group()


def eval_text(fn, gr):
    """The two lines `RNAelem eval` prints (datp: ostream precision 17, vectors as [a,b,...]; motif_eval.hpp:46-47,
    util.hpp:98-105, 175-181)."""
    return "fn: %.17g\n" % fn, "gr: [%s]\n" % ",".join("%.17g" % v for v in gr)


def cmd_eval(a):
    """`eval`: fn / gr of a model file over the whole FASTQ (--no-shuffle semantics: the records as they are); `array-eval`:
    the same over part K of N (arrayjob_manager.hpp:143-151) in the key: value layout that collect_fn_gr_eff reads
    (motif_array_trainer.hpp:20-58).  Note: the reference binary's own `eval` prints zeros -- it never calls set_conditions,
    so its reader hands out no record (tests/golden/eval_text.json) -- ; the format is its, the numbers are the path's."""
    rank, local_rank, world = _rank_world()
    m = io.read_model(a.motif_model)
    if a.lik_ratio:
        m["flags"] |= api.LIK_RATIO
    eng = io.engine_from_model(m, a.device if a.device is not None else local_rank)
    recs = io.read_fastq(a.fastq)
    if a.cmd == "array-eval":
        from .distributed import assigned_range
        tid = a.task_id if a.task_id is not None else int(os.environ.get("SGE_TASK_ID", "1"))
        lo, hi = assigned_range(len(recs), a.array, tid - 1)
        fn, gr, eff = 0.0, np.zeros(eng.n_param), 0.0
        if hi > lo:
            eng.load_batch([s for _, s, _ in recs[lo:hi]], [q for _, _, q in recs[lo:hi]])
            fn, gr, eff, _ = eng.train_eval(m["x"])
        l1, l2 = eval_text(fn, gr)
        with open("%s-%d" % (a.out4, tid), "w") as f:
            f.write("index: %d / %d\nrange: %d - %d\n%s%ssum eff: %.17g\n" % (tid, a.array, lo, hi, l1, l2, eff))
        return
    if world > 1:
        import torch
        import torch.distributed as dist
        torch.cuda.set_device(local_rank)
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("nccl", rank=rank, world_size=world)
    ev = ShardedTrainer(eng, [s for _, s, _ in recs], [q for _, _, q in recs], rank, world,
                        constraints=read_constraints_for(recs, getattr(a, "constraints", None)))
    fn, gr, eff, _ = ev(m["x"])
    if rank == 0:
        l1, l2 = eval_text(fn, gr)
        open(a.out1, "w").write(l1)
        open(a.out2, "w").write(l2)
    if world > 1:
        dist.destroy_process_group()


SUBCOMMANDS = ("train", "scan", "normal", "eval", "array-eval")


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    if not argv or argv[0] not in SUBCOMMANDS + ("-h", "--help"):
        argv = ["normal"] + argv          # the binary without a sub-command (PM_NORMAL, application.hpp:306)
    a = build_parser().parse_args(argv)
    {"train": cmd_train, "normal": cmd_train, "scan": cmd_scan, "eval": cmd_eval, "array-eval": cmd_eval}[a.cmd](a)


if __name__ == "__main__":
    main()
