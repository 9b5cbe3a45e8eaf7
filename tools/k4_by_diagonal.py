"""Durations of the k4_in / k4_out launches of a serial-passes kernel trace, by diagonal:

    rocprofv3 --kernel-trace --stats -d DIR -o run --output-format csv -- python bench.py --steps 2 --warmup 1 --serial-passes
    python tools/k4_by_diagonal.py DIR [W]

On one stream the band launches of a group follow each other: the k-th consecutive k4_in launch of a run is diagonal
k + (W + 1 - launches of the run) (a sweep that skips its first diagonals still ends at W; the launches per run are printed), the
k-th consecutive k4_out launch is diagonal W - k.  Prints, per kernel, the microseconds per diagonal summed over
the groups of the LAST evaluation of the trace, and every other kernel's total over that evaluation.
"""
import csv, glob, os, sqlite3, sys
from collections import defaultdict


def short(n):
    n = n.replace("elemdp::(anonymous namespace)::", "").replace("elemdp::", "").replace("void ", "")
    return n.split("<")[0].split("(")[0].strip()


def form(n):   # the form of the train kernels: sixth template argument = lists, seventh = behind the loop pre-pass (k4_in) / in
    if "<" not in n:   # front of the L kernels (k4_out)
        return ""
    args = n[n.index("<") + 1:n.rindex(">")].replace(" ", "").split(",")
    on = lambda k: len(args) > k and args[k] in ("true", "1")
    return ("lists" if on(5) else "consecutive") + ((" without L" if "k4_out" in n else " behind the pre-pass") if on(6) else "")


def load(d):
    rows = []
    for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            rows.append((r["Kernel_Name"], int(r["Start_Timestamp"]), int(r["End_Timestamp"]), int(r.get("Grid_Size_X") or r.get("Grid_Size") or 0)))
    if rows:
        return sorted(rows, key=lambda r: r[1])
    for f in glob.glob(os.path.join(d, "**", "*.db"), recursive=True):
        c = sqlite3.connect(f)
        cur = c.execute("select * from kernels order by start")
        cols = [x[0] for x in cur.description]
        gx = cols.index("grid_x") if "grid_x" in cols else (cols.index("grid_size_x") if "grid_size_x" in cols else -1)
        for r in cur.fetchall():
            rows.append((r[cols.index("name")], r[cols.index("start")], r[cols.index("end")], r[gx] if gx >= 0 else 0))
    return rows


def main():
    d = sys.argv[1]
    W = int(sys.argv[2]) if len(sys.argv) > 2 else 50
    rows = load(d)
    if not rows:
        sys.exit("no kernel trace under %s" % d)
    # evaluations: each starts with k4_weights
    starts = [k for k, r in enumerate(rows) if short(r[0]) == "k4_weights"]
    ev = rows[starts[-1]:] if starts else rows
    print("kernels in the trace %d, evaluations %d; the last one has %d launches" % (len(rows), len(starts), len(ev)))
    tot = defaultdict(lambda: [0, 0])
    per = {"k4_in": defaultdict(lambda: [0, 0, 0]), "k4_out": defaultdict(lambda: [0, 0, 0])}
    forms = defaultdict(lambda: [0, 0])
    runs = defaultdict(list)
    prev, k = None, 0
    for name, s, e, gx in ev:
        sn = short(name)
        tot[sn][0] += 1; tot[sn][1] += e - s
        if sn in per:
            if prev != sn:
                if prev in per: runs[prev].append(k)
                k = 0
            p = per[sn][k]
            p[0] += 1; p[1] += e - s; p[2] = max(p[2], gx)
            f = forms[sn + " " + form(name)]
            f[0] += 1; f[1] += e - s
            k += 1
        elif prev in per:
            runs[prev].append(k)
        prev = sn
    if prev in per: runs[prev].append(k)
    print("\nper evaluation, all kernels:")
    for sn in sorted(tot, key=lambda x: -tot[x][1]):
        print("  %-22s n %5d  %10.3f ms" % (sn, tot[sn][0], tot[sn][1] / 1e6))
    for f in sorted(forms):
        print("  %-22s n %5d  %10.3f ms" % (f, forms[f][0], forms[f][1] / 1e6))
    for sn in ("k4_in", "k4_out"):
        print("\n%s: launches per run %s" % (sn, sorted(set(runs[sn]))))
        print("  k-th launch of a run: groups, us summed over the groups, largest grid x (threads or workgroups as the trace gives it)")
        for k in sorted(per[sn]):
            p = per[sn][k]
            # the diagonal: a k4_in run that skips its first diagonals ends at W all the same; k4_out runs from W down
            d = k + (W + 1 - max(runs[sn])) if sn == "k4_in" else W - k
            print("  %s launch %2d = d %2d  n %3d  %10.1f us  grid %d" % (sn, k, d, p[0], p[1] / 1e3, p[2]))


if __name__ == "__main__":
    main()
