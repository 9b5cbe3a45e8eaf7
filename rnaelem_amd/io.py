"""On-disk formats either side of the hot path.

  * FASTQ with pseudo-qualities: 4-line records, quality string of length L+1, Sanger offset 33, last
    character '!' <=> the sequence carries the motif        RNAelem/fastq_io.hpp:64-108
  * model text file                                          RNAelem/motif_io.hpp:29-57 (write), :118-262 (read)
  * 10-line scan record                                      RNAelem/motif_scanner.hpp:240-251
  * base-pair posterior record (`scan --out-pairs`; the reference has no such output)
"""
import json
import math

import numpy as np

from . import api

_CODE = np.zeros(256, dtype=np.uint8)
for _c, _v in (("A", 1), ("a", 1), ("C", 2), ("c", 2), ("G", 3), ("g", 3), ("U", 4), ("u", 4), ("T", 4), ("t", 4)):
    _CODE[ord(_c)] = _v
NACGU = "NACGU"


def encode_seq(s):
    """bio_sequence.hpp:28-39: A,C,G,U/T -> 1..4, anything else -> 0."""
    return _CODE[np.frombuffer(s.encode(), dtype=np.uint8)].copy()


def decode_seq(codes):
    return "".join(NACGU[c] for c in codes)


def read_fastq(path, base=33):
    """-> list of (id line incl. '@', code array, quality array).  Like the reference's reader
    (fastq_io.hpp:85-105) a record counts only if all four of its lines are terminated."""
    with open(path) as f:
        lines = f.read().split("\n")
    recs = []
    k = 0
    while k + 4 < len(lines):   # the 4th line must be newline-terminated
        rid, s, _, q = lines[k:k + 4]
        recs.append((rid, encode_seq(s), (np.frombuffer(q.encode(), dtype=np.uint8).astype(np.int16) - base).astype(np.uint8)))
        k += 4
    return recs


def record_name(rid):
    """The name of a FASTQ record or of a constraint record: the id line without its '@' / '>' up to the first blank."""
    f = rid[1:].split()
    return f[0] if f else ""


def read_constraints(path):
    """A FASTA-like file of hard structure constraints, '>id' then the string over api.CONSTRAINT_ALPHABET (it may run over several
    lines) -> {name: string}.  ValueError: text before the first '>', a record without a name, a name given twice."""
    out = {}
    name = None
    with open(path) as f:
        for ln, line in enumerate(f, 1):
            line = line.strip()
            if not line:
                continue
            if line.startswith(">"):
                name = record_name(line)
                if not name:
                    raise ValueError("%s:%d: a constraint record without a name" % (path, ln))
                if name in out:
                    raise ValueError("%s:%d: constraint record %r given twice" % (path, ln, name))
                out[name] = ""
            elif name is None:
                raise ValueError("%s:%d: text before the first '>' line" % (path, ln))
            else:
                out[name] += line
    return out


def constraints_for(recs, cons, path="constraints"):
    """The constraint of every record of read_fastq's list, in its order: the string `cons` (read_constraints) has under the
    record's name, None (free) for a record it does not name.  ValueError: a name no record has, or a string of another length
    than its sequence."""
    names = [record_name(rid) for rid, _, _ in recs]
    unknown = sorted(set(cons) - set(names))
    if unknown:
        raise ValueError("%s: no FASTQ record is named %r" % (path, unknown[0]))
    out = []
    for nm, (_, codes, _) in zip(names, recs):
        c = cons.get(nm)
        if c is not None and len(c) != len(codes):
            raise ValueError("%s: the constraint of %r has %d characters, the sequence %d bases" % (path, nm, len(c), len(codes)))
        out.append(c)
    return out


REQUIRED = ["pattern", "theta|s", "ene-param", "max-span", "rho", "rho-lambda", "tau", "lambda", "min-bpp",
            "max-internal-loop", "theta-softmax"]


def read_model(path):
    """Parse a model file -> dict(pattern, rows, lam, flags, max_span, max_iloop, min_bpp, tau, rho..., ene_param)."""
    d = {}
    for line in open(path):
        line = line.rstrip("\n")
        p = line.split(": ")
        if len(p) < 2:
            continue
        if len(p) != 2:
            raise ValueError("fail to parse: %s" % path)
        d[p[0].strip()] = p[1].strip()
    have = set(d)
    missing = [k for k in REQUIRED if not ((k == "theta|s" and ({"theta", "s"} & have)) or
                                          (k == "rho" and ({"rho-theta", "rho-s"} & have)) or k in have)]
    if missing:
        raise ValueError("motif file broken: %s %s" % (path, missing))
    softmax = bool(int(d["theta-softmax"]))
    no_rss = bool(int(d.get("no-rss", "0")))
    pattern = d["pattern"].replace("_", ".") if no_rss else d["pattern"]
    rows = json.loads(d["s"] if "s" in d else d["theta"])
    m = dict(pattern=pattern, rows=rows, softmax=softmax, lam=json.loads(d["lambda"]), ene_param=d["ene-param"],
             max_span=int(d["max-span"]), max_iloop=int(d["max-internal-loop"]), min_bpp=float(d["min-bpp"]),
             tau=float(d["tau"]), rho_theta=float(d.get("rho-theta", 0)), rho_s=float(d.get("rho-s", 0)),
             rho_lambda=float(d["rho-lambda"]), lambda_prior=float(d.get("lambda-prior", 0)), no_rss=no_rss,
             no_prf=bool(int(d.get("no-profile", "0"))), no_ene=bool(int(d.get("no-energy", "0"))))
    m["flags"] = (api.NO_RSS if m["no_rss"] else 0) | (api.NO_PROFILE if m["no_prf"] else 0) | \
        (api.NO_ENERGY if m["no_ene"] else 0) | (api.THETA_SOFTMAX if softmax else 0)
    m["x"] = np.array([v for row in rows for v in row] + list(m["lam"]), dtype=np.float64)
    return m


def engine_from_model(m, device=-1):
    ene = m["ene_param"]
    par = ene if ene in ("~T2004~", "~A2007~") else open(ene).read()
    return api.Engine(m["pattern"], par, m["max_span"], m["max_iloop"], m["min_bpp"], m["tau"], m["flags"], device)


def fmt(v):
    """Default ostream formatting of a double (6 significant digits), as util.hpp:98-105 prints vectors."""
    if isinstance(v, (int, np.integer)):
        return str(int(v))
    if v == -math.inf:
        return "-inf"
    if v == math.inf:
        return "inf"
    if v != v:
        return "nan"
    return "%.6g" % v


def fmt_vec(v):
    return "[" + ",".join(fmt(x) for x in v) + "]"


def _log_softmax_rows(rows):
    out = []
    for r in rows:
        a = np.array(r, dtype=np.float64)
        mx = a.max()
        out.append(list(a - (mx + math.log(np.exp(a - mx).sum()))))
    return out


def write_model(path, m, x=None):
    """Model file in the reference's layout (RNAelemWriter::write)."""
    rows = m["rows"]
    lam = m["lam"]
    if x is not None:
        k, rows = 0, []
        for r in m["rows"]:
            rows.append(list(x[k:k + len(r)]))
            k += len(r)
        lam = list(x[k:k + 2])
    theta = _log_softmax_rows(rows) if m["softmax"] else rows
    pat = m["pattern"].replace(".", "_") if m["no_rss"] else m["pattern"]
    with open(path, "w") as f:
        f.write("pattern: %s\n" % pat)
        f.write("%s: [%s]\n" % ("s" if m["softmax"] else "theta", ",".join(fmt_vec(r) for r in rows)))
        f.write("exp-theta: [%s]\n" % ",".join(fmt_vec(np.exp(r)) for r in theta))
        f.write("ene-param: %s\nmax-span: %d\nmax-internal-loop: %d\n" % (m["ene_param"], m["max_span"], m["max_iloop"]))
        f.write("theta-softmax: %d\n" % int(m["softmax"]))
        f.write("%s: %s\n" % (("rho-s", fmt(m["rho_s"])) if m["softmax"] else ("rho-theta", fmt(m["rho_theta"]))))
        f.write("rho-lambda: %s\ntau: %s\nlambda: %s\nlambda-prior: %s\nmin-bpp: %s\n" % (
            fmt(m["rho_lambda"]), fmt(m["tau"]), fmt_vec(lam), fmt(m["lambda_prior"]), fmt(m["min_bpp"])))
        f.write("no-rss: %d\nno-profile: %d\nno-energy: %d\n" % (int(m["no_rss"]), int(m["no_prf"]), int(m["no_ene"])))


def scan_record(rid, codes, rec, nodes):
    """The 10-line record of `RNAelem scan` (motif_scanner.hpp:240-251)."""
    M = len(nodes)
    mot = "".join(" " if (h == 0 or h == M - 1) else nodes[h] for h in rec["psihat"])
    return "\n".join([
        "id: " + rid, "start: " + fmt_vec(rec["start"]), "end: " + fmt_vec(rec["end"]), "inner: " + fmt_vec(rec["inner"]),
        "psihat: " + fmt_vec([int(v) for v in rec["psihat"]]), "motif region: %d - %d" % (rec["Ys"], rec["Ye"]),
        "exist prob: " + fmt(rec["exist_prob"]), "seq: " + decode_seq(codes), "rss: " + rec["rss"], "mot: " + mot]) + "\n"


def pair_record(rid, L, pairs, unpaired):
    """Record of one sequence in the `scan --out-pairs` file: its id, the L unpaired probabilities, the number of pairs, then one
    line `i j p` per pair -- 1-based base positions i < j (cell (i0, j0) -> i0+1, j0), ordered by i then j, p as %.6g."""
    ii, jj, pp = pairs
    assert len(unpaired) == L
    lines = ["id: " + rid, "unpaired: " + fmt_vec(unpaired), "pairs: %d" % len(pp)]
    lines += ["%d %d %.6g" % (int(a) + 1, int(b), float(v)) for a, b, v in zip(ii, jj, pp)]
    return "\n".join(lines) + "\n"


def read_pair_records(path):
    """-> list of (id, unpaired array, [(i, j, p), ...] with 1-based i < j) from a `scan --out-pairs` file."""
    lines = open(path).read().split("\n")
    out, k = [], 0
    while k + 2 < len(lines) and lines[k].startswith("id: "):
        rid = lines[k][4:]
        body = lines[k + 1][len("unpaired: "):].strip("[]")
        unp = np.array([float(v) for v in body.split(",")] if body else [])
        n = int(lines[k + 2][len("pairs: "):])
        prs = [(int(a), int(b), float(v)) for a, b, v in (lines[k + 3 + t].split() for t in range(n))]
        out.append((rid, unp, prs))
        k += 3 + n
    return out


def contrast_record(rid, rec):
    """Record of one sequence in the `scan --out-contrast` file, from a record of Engine.conditional_pairs with structures: the id
    line with exist_prob and shift (tab separated, fmt), the maximum expected accuracy structure with the motif and the one
    without it, the two lines of unpaired probabilities, the number of pairs, then one line `i j p_motif p_none` per pair --
    1-based base positions i < j (cell (i0, j0) -> i0+1, j0), ordered by i then j, probabilities as %.6g."""
    lines = ["id: %s\texist prob: %s\tshift: %s" % (rid, fmt(rec["exist_prob"]), fmt(rec["shift"])),
             "motif: " + rec["structure_motif"], "none: " + rec["structure_none"],
             "unpaired motif: " + fmt_vec(rec["unpaired_motif"]), "unpaired none: " + fmt_vec(rec["unpaired_none"]),
             "pairs: %d" % len(rec["i"])]
    lines += ["%d %d %.6g %.6g" % (int(a) + 1, int(b), float(u), float(v))
              for a, b, u, v in zip(rec["i"], rec["j"], rec["p_motif"], rec["p_none"])]
    return "\n".join(lines) + "\n"


def read_contrast_records(path):
    """-> list of dicts (id, exist_prob, shift, structure_motif, structure_none, unpaired_motif, unpaired_none,
    pairs = [(i, j, p_motif, p_none), ...] with 1-based i < j) from a `scan --out-contrast` file."""
    lines = open(path).read().split("\n")
    out, k = [], 0

    def vec(line, head):
        if not line.startswith(head):
            raise ValueError("contrast record: line %r where %r was expected" % (line, head))
        body = line[len(head):].strip("[]")
        return np.array([float(v) for v in body.split(",")] if body else [])

    while k + 5 < len(lines) and lines[k].startswith("id: "):
        rid, ex, sh = lines[k][4:].rsplit("\t", 2)
        n = int(lines[k + 5][len("pairs: "):])
        prs = [(int(a), int(b), float(u), float(v)) for a, b, u, v in (lines[k + 6 + t].split() for t in range(n))]
        out.append(dict(id=rid, exist_prob=float(ex[len("exist prob: "):]), shift=float(sh[len("shift: "):]),
                        structure_motif=lines[k + 1][len("motif: "):], structure_none=lines[k + 2][len("none: "):],
                        unpaired_motif=vec(lines[k + 3], "unpaired motif: "), unpaired_none=vec(lines[k + 4], "unpaired none: "),
                        pairs=prs))
        k += 6 + n
    return out


def mea_record(rid, structure, score):
    """Record of one sequence in the `scan --out-mea` file: its id, the maximum expected accuracy structure under the motif model
    ('(', ')', '.'; one character per base) and its score as %.17g."""
    return "id: %s\nmea: %s\nscore: %.17g\n" % (rid, structure, float(score))


def read_mea_records(path):
    """-> list of (id, structure, score) from a `scan --out-mea` file."""
    lines = open(path).read().split("\n")
    out, k = [], 0
    while k + 2 < len(lines) and lines[k].startswith("id: "):
        out.append((lines[k][4:], lines[k + 1][len("mea: "):], float(lines[k + 2][len("score: "):])))
        k += 3
    return out


def sample_motif_span(nodes, M):
    """(start, end) of the motif in one sample, half-open: the span of the positions whose node is neither 0 nor M-1 (the non-blank
    part of `mot`), or (-1, -1) when the sample has no motif."""
    inside = [p for p, h in enumerate(nodes) if h != 0 and h != M - 1]
    return (inside[0], inside[-1] + 1) if inside else (-1, -1)


SAMPLE_STATUS = ("sampled", "no parse", "refused")


def sample_record(rid, samples, nodes, status=0):
    """Record of one sequence in the `scan --out-samples` file: `id: <id>`, `samples: N`, then one line per sample with the
    tab-separated fields index, log-probability (%.17g), motif start and end (half-open, 0-based; -1 -1 without a motif),
    dot-bracket (L -> '(', R -> ')', else '.'), the structure letters, and the `mot` string of scan_record (the node name per
    position, blank outside the motif).  samples: (rss strings, node rows, logps) as Engine.sample_structures gives them for a
    sampled sequence, or None (N = 0: not sampled); nodes: the pattern's node names.  A line `status: <sampled | no parse |
    refused>` (Engine.sample_structures' status) follows the count."""
    rss, node, logp = samples if samples is not None else ([], [], [])
    M = len(nodes)
    lines = ["id: " + rid, "samples: %d" % len(rss), "status: " + SAMPLE_STATUS[status]]
    for t, (r, h, lp) in enumerate(zip(rss, node, logp)):
        a, b = sample_motif_span(h, M)
        db = "".join("(" if c == "L" else ")" if c == "R" else "." for c in r)
        mot = "".join(" " if (v == 0 or v == M - 1) else nodes[v] for v in h)
        lines.append("\t".join([str(t), "%.17g" % float(lp), str(a), str(b), db, r, mot]))
    return "\n".join(lines) + "\n"


def read_sample_records(path):
    """-> list of (id, status, [(index, logp, start, end, dot-bracket, rss, mot), ...]) from a `scan --out-samples` file."""
    lines = open(path).read().split("\n")
    out, k = [], 0
    while k + 1 < len(lines) and lines[k].startswith("id: "):
        rid = lines[k][4:]
        n = int(lines[k + 1][len("samples: "):])
        status = lines[k + 2][len("status: "):]
        rows = []
        for t in range(n):
            f = lines[k + 3 + t].split("\t")
            rows.append((int(f[0]), float(f[1]), int(f[2]), int(f[3]), f[4], f[5], f[6]))
        out.append((rid, status, rows))
        k += 3 + n
    return out


CONTEXT_LETTERS = "OLRHBIM"


def context_record(rid, profile):
    """Record of one sequence in the `scan --out-context` file: `id: <id>`, then seven lines `O: [...]` to `M: [...]` with the
    probability of that structure letter at every base (6 significant digits); profile: an (L, 7) array as
    Engine.context_profiles gives it."""
    profile = np.asarray(profile, dtype=np.float64).reshape(-1, len(CONTEXT_LETTERS))
    lines = ["id: " + rid] + ["%s: %s" % (c, fmt_vec(profile[:, k])) for k, c in enumerate(CONTEXT_LETTERS)]
    return "\n".join(lines) + "\n"


def read_context_records(path):
    """-> list of (id, (L, 7) array) from a `scan --out-context` file."""
    lines = open(path).read().split("\n")
    out, k = [], 0
    n = len(CONTEXT_LETTERS)
    while k + n < len(lines) and lines[k].startswith("id: "):
        cols = []
        for t, c in enumerate(CONTEXT_LETTERS):
            head, body = lines[k + 1 + t].split(": ", 1)
            if head != c:
                raise ValueError("context record %r: line %r where %r was expected" % (lines[k][4:], head, c))
            body = body.strip("[]")
            cols.append([float(v) for v in body.split(",")] if body else [])
        out.append((lines[k][4:], np.array(cols, dtype=np.float64).T.reshape(-1, n)))
        k += 1 + n
    return out


def access_record(rid, access):
    """Record of one sequence in the `scan --out-access` file: `id: <id>`, then one line per width `u1: [...]` .. `uU: [...]` with
    the probability that the window of that width starting at every base is unpaired (6 significant digits; `nan` where the
    window runs off the end); access: an (L, U) array as Engine.accessibility gives it."""
    access = np.asarray(access, dtype=np.float64)
    lines = ["id: " + rid] + ["u%d: %s" % (w + 1, fmt_vec(access[:, w])) for w in range(access.shape[1])]
    return "\n".join(lines) + "\n"


def read_access_records(path):
    """-> list of (id, (L, U) array) from a `scan --out-access` file."""
    lines = open(path).read().split("\n")
    out, k = [], 0
    while k < len(lines) and lines[k].startswith("id: "):
        rid = lines[k][4:]
        k += 1
        cols = []
        while k < len(lines) and lines[k] and not lines[k].startswith("id: "):
            head, body = lines[k].split(": ", 1)
            if head != "u%d" % (len(cols) + 1):
                raise ValueError("access record %r: line %r where u%d was expected" % (rid, head, len(cols) + 1))
            body = body.strip("[]")
            cols.append([float(v) for v in body.split(",")] if body else [])
            k += 1
        out.append((rid, np.array(cols, dtype=np.float64).T.reshape(-1, len(cols))))
    return out


def node_record(rid, profile, names, confidence=None):
    """Record of one sequence in the `scan --out-nodes` file: `id: <id>`, then one line per pattern node `<index><name>: [...]`
    with the probability that the node emits each base (6 significant digits); profile: an (L, M) array as Engine.node_profiles
    gives it, names: describe()["node"].  confidence (api.alignment_confidence of the scan's psihat) adds a last line
    `confidence: [...]`."""
    M = len(names)
    profile = np.asarray(profile, dtype=np.float64).reshape(-1, M)
    lines = ["id: " + rid] + ["%d%s: %s" % (k, c, fmt_vec(profile[:, k])) for k, c in enumerate(names)]
    if confidence is not None:
        lines.append("confidence: " + fmt_vec(confidence))
    return "\n".join(lines) + "\n"


def read_node_records(path):
    """-> list of (id, node names, (L, M) array, confidence or None) from a `scan --out-nodes` file."""
    def vec(body):
        body = body.strip("[]")
        return [float(v) for v in body.split(",")] if body else []

    lines = open(path).read().split("\n")
    out, k = [], 0
    while k < len(lines) and lines[k].startswith("id: "):
        rid = lines[k][4:]
        k += 1
        names, cols, conf = "", [], None
        while k < len(lines) and lines[k] and not lines[k].startswith("id: "):
            head, body = lines[k].split(": ", 1)
            if head == "confidence":
                conf = np.array(vec(body), dtype=np.float64)
            else:
                if not head[:-1].isdigit() or int(head[:-1]) != len(cols):
                    raise ValueError("node record %r: line %r where node %d was expected" % (rid, head, len(cols)))
                names += head[-1]
                cols.append(vec(body))
            k += 1
        out.append((rid, names, np.array(cols, dtype=np.float64).T.reshape(-1, len(cols)), conf))
    return out


def site_record(rid, res, names):
    """Record of one sequence in the `scan --out-sites` file: `id: <id>`, then per site k one line `site k: start end score
    confidence` (the region [start, end) that carries the pattern's nodes, the score of the whole row, the mean of N(p, row[p])
    over the site; 6 significant digits) and one line with the node name of every base; res: one entry of
    Engine.mea_alignments, names: describe()["node"].  A sequence without a site has the id line alone."""
    lines = ["id: " + rid]
    for k in range(len(res["start"])):
        lines.append("site %d: %d %d %s %s" % (k, res["start"][k], res["end"][k], fmt(float(res["score"][k])), fmt(float(res["confidence"][k]))))
        lines.append("".join(names[int(m)] for m in res["rows"][k]))
    return "\n".join(lines) + "\n"


def read_sites(path):
    """-> list of (id, dict(start, end, score, confidence, rows)) from a `scan --out-sites` file; rows: the lines of node names."""
    lines = open(path).read().split("\n")
    out, k = [], 0
    while k < len(lines) and lines[k].startswith("id: "):
        rid = lines[k][4:]
        k += 1
        start, end, score, conf, rows = [], [], [], [], []
        while k < len(lines) and lines[k].startswith("site "):
            head, body = lines[k].split(": ", 1)
            if int(head[5:]) != len(start):
                raise ValueError("site record %r: line %r where site %d was expected" % (rid, head, len(start)))
            a, b, sc, cf = body.split()
            start.append(int(a)); end.append(int(b)); score.append(float(sc)); conf.append(float(cf))
            rows.append(lines[k + 1])
            k += 2
        out.append((rid, dict(start=np.array(start, dtype=np.int32), end=np.array(end, dtype=np.int32), score=np.array(score),
                              confidence=np.array(conf), rows=rows)))
    return out


def logo_counts_record(rid, exist_prob, counts):
    """Record of one sequence on the way to the `scan --out-logo` file: `id: <id>`, `exist: <exist_prob>` and `counts: [...]`, the
    sequence's (M, 7, 5) block of Engine.joint_profiles in full precision: the ranks of a sharded run write these, and rank 0
    joins them in input order before it sums."""
    counts = np.asarray(counts, dtype=np.float64)
    return "id: %s\nexist: %.17g\ncounts: [%s]\n" % (rid, exist_prob, ",".join("%.17g" % v for v in counts.ravel()))


def read_logo_counts(path):
    """-> list of (id, exist_prob, (M, 7, 5) array) from the per-sequence records of logo_counts_record."""
    lines = open(path).read().split("\n")
    out, k = [], 0
    while k + 2 < len(lines) and lines[k].startswith("id: "):
        if not lines[k + 1].startswith("exist: ") or not lines[k + 2].startswith("counts: "):
            raise ValueError("logo counts record %r: exist and counts lines expected" % lines[k][4:])
        body = lines[k + 2][8:].strip("[]")
        v = np.array([float(t) for t in body.split(",")] if body else [], dtype=np.float64)
        out.append((lines[k][4:], float(lines[k + 1][7:]), v.reshape(-1, 7, 5)))
        k += 3
    return out


LOGO_BASES = "NACGU"


def write_logo(path, names, counts, n_used, n_total=None):
    """The `scan --out-logo` file: a header `sequences: <used> / <read>` and `columns: N A C G U`, then one record per pattern node:
    `node: <index><name>`, `occurrences: <expected number of bases the node emits>` and seven lines `O: [...]` .. `M: [...]`, the
    node's expected emission counts of each base under that structure letter (17 significant digits: the file is a sum that
    further sums are formed from); counts: an (M, 7, 5) array, the `counts` of api.motif_logo."""
    counts = np.asarray(counts, dtype=np.float64).reshape(len(names), 7, 5)
    lines = ["sequences: %d / %d" % (n_used, n_used if n_total is None else n_total), "columns: " + " ".join(LOGO_BASES)]
    for m, c in enumerate(names):
        lines += ["node: %d%s" % (m, c), "occurrences: %.17g" % counts[m].sum()]
        lines += ["%s: [%s]" % (l, ",".join("%.17g" % v for v in counts[m, k])) for k, l in enumerate(CONTEXT_LETTERS)]
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


def read_logo(path):
    """-> dict(n_used, n_total, names, occurrences (M,), counts (M, 7, 5)) from a `scan --out-logo` file."""
    lines = open(path).read().split("\n")
    if len(lines) < 2 or not lines[0].startswith("sequences: ") or lines[1] != "columns: " + " ".join(LOGO_BASES):
        raise ValueError("logo file %r: header expected" % path)
    used, total = (int(t) for t in lines[0][11:].split(" / "))
    names, occ, blocks = "", [], []
    k = 2
    while k < len(lines) and lines[k].startswith("node: "):
        head = lines[k][6:]
        if not head[:-1].isdigit() or int(head[:-1]) != len(blocks) or not lines[k + 1].startswith("occurrences: "):
            raise ValueError("logo file %r: record of node %d expected at line %d" % (path, len(blocks), k + 1))
        names += head[-1]
        occ.append(float(lines[k + 1][13:]))
        rows = []
        for t, l in enumerate(CONTEXT_LETTERS):
            h, body = lines[k + 2 + t].split(": ", 1)
            if h != l:
                raise ValueError("logo file %r: line %r where %r was expected" % (path, h, l))
            rows.append([float(v) for v in body.strip("[]").split(",")])
        blocks.append(rows)
        k += 2 + len(CONTEXT_LETTERS)
    return dict(n_used=used, n_total=total, names=names, occurrences=np.array(occ), counts=np.array(blocks, dtype=np.float64).reshape(-1, 7, 5))


def stem_counts_record(rid, exist_prob, counts):
    """Record of one sequence on the way to the `scan --out-stems` file: `id: <id>`, `exist: <exist_prob>` and `stems: [...]`, the
    sequence's (K, 5, 5) block of Engine.stem_profiles in full precision: the ranks of a sharded run write these, and rank 0
    joins them in input order before it sums."""
    counts = np.asarray(counts, dtype=np.float64)
    return "id: %s\nexist: %.17g\nstems: [%s]\n" % (rid, exist_prob, ",".join("%.17g" % v for v in counts.ravel()))


def read_stem_counts(path):
    """-> list of (id, exist_prob, (K, 5, 5) array) from the per-sequence records of stem_counts_record."""
    lines = open(path).read().split("\n")
    out, k = [], 0
    while k + 2 < len(lines) and lines[k].startswith("id: "):
        if not lines[k + 1].startswith("exist: ") or not lines[k + 2].startswith("stems: "):
            raise ValueError("stem counts record %r: exist and stems lines expected" % lines[k][4:])
        body = lines[k + 2][7:].strip("[]")
        v = np.array([float(t) for t in body.split(",")] if body else [], dtype=np.float64)
        out.append((lines[k][4:], float(lines[k + 1][7:]), v.reshape(-1, 5, 5)))
        k += 3
    return out


def stem_pair_line(rid, i, j, left, right, q):
    """One line of the `scan --out-stem-pairs` file: the sequence id, the 1-based positions i < j of the two paired bases
    (as the `scan --out-pairs` file numbers them: cell (i0, j0) -> i0+1, j0), the two pattern nodes that emit them as `<index><name>` and the probability q of that labelled pair."""
    return "%s\t%d\t%d\t%s\t%s\t%.6g\n" % (rid, i, j, left, right, q)


def helix_line(rid, i, j, n, p):
    """One line of the `scan --out-helices` file: the sequence id, the 1-based positions i < j of the two bases of the outermost
    pair (as the `scan --out-stem-pairs` file numbers them: cell (i0, j0) -> i0+1, j0), the number n of directly stacked pairs
    (i, j), (i+1, j-1), .. and the probability p that all of them form."""
    return "%s\t%d\t%d\t%d\t%.6g\n" % (rid, i, j, n, p)


def read_helices(path):
    """-> list of dict(id, i, j, len, p) from a `scan --out-helices` file, i 0-based and j exclusive (the engine's cells)."""
    out = []
    for line in open(path).read().split("\n")[:-1]:
        f = line.split("\t")
        if len(f) != 5:
            raise ValueError("helices file %r: five fields expected in %r" % (path, line))
        out.append(dict(id=f[0], i=int(f[1]) - 1, j=int(f[2]), len=int(f[3]), p=float(f[4])))
    return out


def mea_helix_line(rid, i, j, n, p_joint, p_min):
    """One line of the `scan --out-mea-helices` file, a stem of the sequence's maximum expected accuracy structure: the fields of
    helix_line with the joint probability of the whole stem, then the smallest pair posterior in it."""
    return "%s\t%d\t%d\t%d\t%.6g\t%.6g\n" % (rid, i, j, n, p_joint, p_min)


def read_mea_helices(path):
    """-> list of dict(id, i, j, len, p, p_min) from a `scan --out-mea-helices` file, i 0-based and j exclusive."""
    out = []
    for line in open(path).read().split("\n")[:-1]:
        f = line.split("\t")
        if len(f) != 6:
            raise ValueError("MEA helices file %r: six fields expected in %r" % (path, line))
        out.append(dict(id=f[0], i=int(f[1]) - 1, j=int(f[2]), len=int(f[3]), p=float(f[4]), p_min=float(f[5])))
    return out


LOOP_LETTERS = "HSBIM"


def loop_line(rid, letter, i, j, k, l, p):
    """One line of the `scan --out-loops` file: the sequence id, the type letter of the loop (H hairpin, S stack, B bulge, I interior
    loop, M multi-branch loop), the 1-based positions i < j of the two bases of the closing pair (as the `scan --out-helices` file
    numbers them: cell (i0, j0) -> i0+1, j0), the 1-based positions k < l of the two bases of the inner pair of a two-loop (None:
    `-`, the closing rows of the types H, S and M), and the probability."""
    kl = "-\t-" if k is None else "%d\t%d" % (k, l)
    return "%s\t%s\t%d\t%d\t%s\t%.6g\n" % (rid, letter, i, j, kl, p)


def loop_lines(rid, closing, two):
    """The lines of one sequence in the `scan --out-loops` file from its closing list (i, j, p, cols) and its two-loop list
    (i, j, k, l, p) of Engine.loop_posteriors: per closing cell the rows H, S and M of the columns that are not 0, then the cell's
    two-loops as rows B or I.  Both lists are in (i, j) order of the outer cell; a two-loop whose outer cell has no closing
    row (its pair posterior within rounding below the threshold) is written in its place in that order."""
    ii, jj, _, cols = closing
    ti, tj, tk, tl, tp = two
    out, t = [], 0

    def two_rows(upto):   # the two-loops whose outer cell is at or before `upto` in (i, j) order (None: all that are left)
        nonlocal t
        while t < len(ti) and (upto is None or (ti[t], tj[t]) <= upto):
            bulge = (tk[t] == ti[t] + 1) != (tl[t] == tj[t] - 1)
            out.append(loop_line(rid, "B" if bulge else "I", ti[t] + 1, tj[t], tk[t] + 1, tl[t], tp[t]))
            t += 1

    for i, j, c in zip(ii, jj, cols):
        two_rows((i, j - 1))      # (an outer cell within rounding below the threshold has two-loops but no closing row)
        out += [loop_line(rid, LOOP_LETTERS[w], i + 1, j, None, None, c[w]) for w in (0, 1, 4) if c[w] > 0.0]
        two_rows((i, j))
    two_rows(None)
    return "".join(out)


def _read_loop_fields(path, line, n):
    f = line.split("\t")
    if len(f) != n or f[1] not in LOOP_LETTERS or (f[4] == "-") != (f[5] == "-") or (f[4] == "-") != (f[1] in "HSM"):
        raise ValueError("loops file %r: %d fields with a type letter expected in %r" % (path, n, line))
    two = f[4] != "-"
    return dict(id=f[0], type=f[1], i=int(f[2]) - 1, j=int(f[3]), k=int(f[4]) - 1 if two else None, l=int(f[5]) if two else None,
                p=float(f[6]))


def read_loops(path):
    """-> list of dict(id, type, i, j, k, l, p) from a `scan --out-loops` file, i and k 0-based, j and l exclusive (the engine's
    cells); k and l are None on the rows of the types H, S and M."""
    return [_read_loop_fields(path, line, 7) for line in open(path).read().split("\n")[:-1]]


def mea_loop_line(rid, letter, i, j, k, l, p_loop, p_pair):
    """One line of the `scan --out-mea-loops` file, a loop of the sequence's maximum expected accuracy structure: the fields of
    loop_line with the probability of the loop, then the pair posterior of its closing pair."""
    return loop_line(rid, letter, i, j, k, l, p_loop)[:-1] + "\t%.6g\n" % p_pair


def read_mea_loops(path):
    """-> list of dict(id, type, i, j, k, l, p, p_pair) from a `scan --out-mea-loops` file, cells as read_loops."""
    out = []
    for line in open(path).read().split("\n")[:-1]:
        r = _read_loop_fields(path, line, 8)
        r["p_pair"] = float(line.split("\t")[7])
        out.append(r)
    return out


def write_stems(path, names, slots, counts, n_used, n_total=None):
    """The `scan --out-stems` file: a header `sequences: <used> / <read>` and `columns: N A C G U`, then one record per stem slot:
    `stem: <index><name> <index><name>` (the pattern nodes of the left and the right base), `occurrences: <expected number of
    pairs>` and five lines `N: [...]` .. `U: [...]`, the row of a left base over the right bases (17 significant digits: the
    file is a sum that further sums are formed from); slots: (K, 2) node indices; counts: a (K, 5, 5) array."""
    slots = np.asarray(slots, dtype=np.int64).reshape(-1, 2)
    counts = np.asarray(counts, dtype=np.float64).reshape(len(slots), 5, 5)
    lines = ["sequences: %d / %d" % (n_used, n_used if n_total is None else n_total), "columns: " + " ".join(LOGO_BASES)]
    for k, (l, r) in enumerate(slots):
        lines += ["stem: %d%s %d%s" % (l, names[l], r, names[r]), "occurrences: %.17g" % counts[k].sum()]
        lines += ["%s: [%s]" % (b, ",".join("%.17g" % v for v in counts[k, t])) for t, b in enumerate(LOGO_BASES)]
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


def read_stems(path):
    """-> dict(n_used, n_total, slots (K, 2), names (K pairs of node names), occurrences (K,), counts (K, 5, 5)) from a
    `scan --out-stems` file."""
    lines = open(path).read().split("\n")
    if len(lines) < 2 or not lines[0].startswith("sequences: ") or lines[1] != "columns: " + " ".join(LOGO_BASES):
        raise ValueError("stems file %r: header expected" % path)
    used, total = (int(t) for t in lines[0][11:].split(" / "))
    slots, names, occ, blocks = [], [], [], []
    k = 2
    while k < len(lines) and lines[k].startswith("stem: "):
        heads = lines[k][6:].split(" ")
        if len(heads) != 2 or not all(h[:-1].isdigit() for h in heads) or not lines[k + 1].startswith("occurrences: "):
            raise ValueError("stems file %r: record of slot %d expected at line %d" % (path, len(blocks), k + 1))
        slots.append([int(h[:-1]) for h in heads])
        names.append((heads[0][-1], heads[1][-1]))
        occ.append(float(lines[k + 1][13:]))
        rows = []
        for t, b in enumerate(LOGO_BASES):
            h, body = lines[k + 2 + t].split(": ", 1)
            if h != b:
                raise ValueError("stems file %r: line %r where %r was expected" % (path, h, b))
            rows.append([float(v) for v in body.strip("[]").split(",")])
        blocks.append(rows)
        k += 2 + len(LOGO_BASES)
    return dict(n_used=used, n_total=total, slots=np.array(slots, dtype=np.int64).reshape(-1, 2), names=names, occurrences=np.array(occ),
                counts=np.array(blocks, dtype=np.float64).reshape(-1, 5, 5))
