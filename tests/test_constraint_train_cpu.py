"""The enumeration reference of a constrained train row (tests/constraint_train_check.py) justified by the
oracle alone, without a GPU: the mixture over ALL structures reproduces the free oracle's row; the routes every string gets are
counted and capped; the partition identity among enumerated references; and a self-test of what the per-sequence comparison sees
and the batch gradient at its tolerance does not."""
import numpy as np
import pytest

from oracle import pyoracle as po
from tests import constraint_check as kc
from tests import constraint_train_check as kt
from tests import joint_check as jc
from tests import train_check as tc

Z_TOL = 1e-12                             # ln Z of the mixture against the free oracle's
C_RTOL, C_ATOL = 1e-10, 1e-12             # counts of the mixture against the free oracle's
WORST = dict(z=0.0, count=0.0)            # the largest errors test_free_row has seen, in units of the bounds above


@pytest.fixture(scope="module")
def cases():
    return kt.train_cases()


def flag_sets(case):
    """the case's own flags; LIK_RATIO as well on the first quoted case (flags 0)"""
    return [case[2]] + ([case[2] | po.LIK_RATIO] if case == kc.QUOTED[0][0] else [])


def close(got, ref, rtol, atol, what):
    err = tc.count_error(got, ref, rtol, atol)
    assert err.max() <= rtol, "%s: error %.3e of rtol %.1e / atol %.1e" % (what, err.max(), rtol, atol)
    return float(err.max()) / rtol


# ---- 1. the free row

def test_free_row(cases):
    """The string of all '.' is satisfied by every structure, so the mixture over all structures must be the free oracle's row.
    Every enumerated case holds structures without a parse with the motif (the one without a pair at least), which the
    fixed-structure oracle skips: the Zari-weighted vectors (ENx, EHx with the motif; ENo, EHo without it under LIK_RATIO) are
    compared in full.  For the Zo- and Znasi-weighted vectors the sum over the structures that are not skipped falls short of the
    free row by the skipped ones' share, sum over skipped s of Z_s B_s with Zo_s = Znasi_s: the SAME shortfall for ENo with the
    motif, ENo without it and ENx without it, each in units of its own Z.  That the three agree is what the direct and the
    complement route rest on."""
    n_vec = 0
    for case, x, s, q, _, _ in cases:
        for flags in flag_sets(case):
            dbs, _ = kt.case_structures(case, flags, x, s)
            short = {}
            for last in kt.LABELS:
                ql = kt.labelled(q, last)
                what = (case, flags, tc.label(ql))
                free = kt.free_row(case, flags, x, s, ql)
                rows = kt.structure_rows(case, flags, x, s, ql, dbs)
                every = [rows[db] for db in dbs]
                m = kt.mixture_row(flags, ql, every, [], free, complement_ok=False, force="direct")
                for key in kt.ZKEYS:
                    err = abs(m[key] - free[key]) / max(1.0, abs(free[key]))
                    WORST["z"] = max(WORST["z"], err / Z_TOL)
                    assert err <= Z_TOL, (what, key, m[key], free[key])
                assert m["skipped"] == free["skipped"] == 0 and abs(m["f"] - free["f"]) <= 2 * Z_TOL * max(1.0, abs(free["Zo"])), what
                zo_key, zx_key, _ = kt.ensemble_keys(flags, tc.has_motif(ql))
                assert "Zari" not in (zo_key, zx_key) or m["parts"]["o" if zo_key == "Zari" else "x"] == "direct", what
                for key in tc.COUNTS:
                    if key in m:
                        WORST["count"] = max(WORST["count"], close(m[key], free[key], C_RTOL, C_ATOL, "%s %s" % (what, key)))
                        n_vec += 1
                for zkey, keys in ((zo_key, ("ENo", "EHo")), (zx_key, ("ENx", "EHx"))):
                    if zkey == "Zari":
                        continue
                    assert kt.lost(every, zkey), what          # (else the direct route above served these vectors)
                    part = kt.weighted(every, zkey, free[zkey], keys)
                    # in units of Zo: the shortfall times Z / Zo
                    short[(last, keys[0])] = [(free[k] - v) * np.exp(free[zkey] - free["Zo"]) for k, v in zip(keys, part)]
            if not flags & po.LIK_RATIO:
                a, b, c = short[(0, "ENo")], short[(5, "ENo")], short[(5, "ENx")]
                assert max(np.abs(a[0]).max(), np.abs(a[1]).max()) > 0
                for other, name in ((b, "ENo without the motif"), (c, "ENx without the motif")):
                    for u, v, vec in zip(other, a, ("EN", "EH")):
                        WORST["count"] = max(WORST["count"], close(u, v, C_RTOL, C_ATOL, "%s shortfall of %s %s" % (case, name, vec)))
    assert n_vec >= 2 * (len(cases) + 2)
    print("free row: largest error of ln Z %.2e, of a count %.2e of its bound (rtol %g, atol %g)" % (
        WORST["z"] * Z_TOL, WORST["count"], C_RTOL, C_ATOL))


# ---- 2. the routes

def routes_of(case, x, s, q, c, e):
    """the route of the Zo-weighted and of the Znasi-weighted vectors of a string, or "unsatisfiable" / "skipped" """
    r0 = kt.constrained_row(case, x, s, q, c, e, 0)
    r5 = kt.constrained_row(case, x, s, q, c, e, 5)
    if not np.isfinite(r0["Zo"]):
        return "unsatisfiable"
    if r0["skipped"]:
        return "skipped"
    assert r0["parts"]["x"] == "direct" and r0["parts"]["o"] == r5["parts"]["o"]          # the A part is always there
    got = {r5["parts"]["o"], r5["parts"]["x"]}
    return None if None in got else "complement" if "complement" in got else "direct"


def test_every_string_has_its_routes(cases):
    """A condition on the inputs, not a measurement: every satisfiable quoted string gets all four vectors under both labels, and
    of the strings this module draws for the cases of joint_check.CASES at most one in four is left with the Zari-weighted
    vectors only."""
    quoted = {}
    drawn, own = [], []
    for case, x, s, q, refs, n_own in cases:
        for k, (c, e) in enumerate(refs):
            r = routes_of(case, x, s, q, c, e)
            if case in [qc[0] for qc in kc.QUOTED]:
                quoted[c] = r
            else:
                (own if k < n_own else drawn).append(r)
    assert quoted.pop("...x....x.......") == "complement" and quoted.pop("....xxxx............") == "complement"
    assert quoted.pop("..........|.........") == "unsatisfiable"
    assert len(quoted) == 8 and set(quoted.values()) == {"direct"}, quoted
    print("routes of the drawn strings: %s; of the cases' own strings: %s" % (
        {r: drawn.count(r) for r in set(drawn)}, {r: own.count(r) for r in set(own)}))
    assert len(drawn) >= 2 * len(jc.CASES) - 2
    assert 4 * drawn.count(None) <= len(drawn), drawn
    assert drawn.count("direct") + drawn.count("complement") >= len(drawn) // 2


def test_mixed_z_equals_the_enumeration(cases):
    """Zo, Zari, Znasi of the mixture against constraint_check's own sums over derivation_logz (another call of the oracle)"""
    for case, x, s, q, refs, _ in cases:
        for c, e in refs:
            row = kt.constrained_row(case, x, s, q, c, e, 0)
            assert np.isneginf(row["Zo"]) == np.isneginf(e["lnZ"]) and (not np.isfinite(e["lnZ"]) or abs(row["Zo"] - e["lnZ"]) <= 1e-12 * max(1.0, abs(e["lnZ"])))
            for key in ("Zari", "Znasi"):
                if key in e:
                    assert np.isneginf(row[key]) == np.isneginf(e[key]), (case, c, key)
                    assert not np.isfinite(e[key]) or abs(row[key] - e[key]) <= 1e-12 * max(1.0, abs(e[key])), (case, c, key)


# ---- 3. the partition identity among enumerated references

@pytest.mark.parametrize("which", [0, 1])
def test_partition_identity_of_the_references(which, cases):
    """Z X_free = Z_x X_x + Z_| X_| at one base per quoted sequence (the base whose unpaired probability is nearest 1/2), per
    vector with its own ensemble's Z.  The structure without a pair satisfies x, so the Zo- and Znasi-weighted vectors of x come by the complement route, whose rest is the | string's
    set: for them the identity says that the two routes were put together consistently; for the Zari-weighted vectors it is
    three independent mixtures."""
    case, x, s, q, _, _ = cases[len(jc.CASES) + which]
    assert case == kc.QUOTED[which][0]
    L = len(s)
    o = kt.case_oracle(case, case[2], x)
    dbs, _ = kt.case_structures(case, case[2], x, s)
    srows = kt.structure_rows(case, case[2], x, s, kt.labelled(q, 0), dbs)
    zo = kt.logsum([srows[db]["Zo"] for db in dbs])
    u = np.array([sum(np.exp(srows[db]["Zo"] - zo) for db in dbs if db[p] == ".") for p in range(L)])
    p = int(np.argmin(np.abs(u - 0.5)))
    # (the hairpin of the first sequence leaves no base in mid-range: 4.6e-3 there, enough for the complement route of x)
    assert 4 * kt.MIN_SHARE <= u[p] <= 1 - 4 * kt.MIN_SHARE, u
    strings = ["." * p + ch + "." * (L - p - 1) for ch in "x|"]
    es = [kc.enumerated(o, s, q, c) for c in strings]
    assert min(e["n_sat"] for e in es) >= 2 and es[0]["n_sat"] + es[1]["n_sat"] == es[0]["n_all"]
    for last in kt.LABELS:
        ql = kt.labelled(q, last)
        free = kt.free_row(case, case[2], x, s, ql)
        rx, rp = (kt.constrained_row(case, x, s, q, c, e, last) for c, e in zip(strings, es))
        assert kt.complete(rx) and kt.complete(rp) and rp["parts"]["o"] == "direct", (rx["parts"], rp["parts"])
        zo_key, zx_key, _ = kt.ensemble_keys(case[2], tc.has_motif(ql))
        for zkey, keys in ((zo_key, ("ENo", "EHo")), (zx_key, ("ENx", "EHx"))):
            ax, ap = np.exp(rx[zkey] - free[zkey]), np.exp(rp[zkey] - free[zkey])
            assert abs(ax + ap - 1.0) <= 1e-12 and 1e-4 < ax < 1 - 1e-4, (ax, ap)
            for key in keys:
                np.testing.assert_allclose(ax * rx[key] + ap * rp[key], free[key], rtol=1e-12, atol=1e-12, err_msg="%s %s" % (tc.label(ql), key))


# ---- 4. what the per-sequence comparison sees

def test_checker_sees_a_structure_the_batch_gradient_hides(cases):
    """A kernel whose `unp` test fails lets a structure through that does not satisfy the string.  The row of the string
    `(............)..` with the motif, with one such structure added at its weight: there is a structure for which the batch
    gradient of the case's batch stays within GR_TOL (ENo and ENx move together: gr holds the difference, pn (B - A)), while
    compare_counts names the sequence."""
    case, x, s, q, refs, _ = cases[len(jc.CASES)]
    c, e = refs[2]
    assert c == "(............).."
    (seqs, quals, cons, rows), _ = kt.batch_of(case, x, s, q, refs)
    k = [j for j in range(len(seqs)) if cons[j] == c and tc.has_motif(quals[j])][0]
    good = rows[k]
    assert kt.complete(good) and not good["skipped"]
    ql = quals[k]
    dbs, _ = kt.case_structures(case, case[2], x, s)
    srows = kt.structure_rows(case, case[2], x, s, ql, dbs)
    gr_ref = kt.gr_of(rows, len(x))
    found = None
    for db in dbs:
        r = srows[db]
        if kc.satisfies(db, c) or r["skipped"]:
            continue
        bad = dict(good)
        for zkey, keys in (("Zo", ("ENo", "EHo")), ("Zari", ("ENx", "EHx"))):
            z = np.logaddexp(good[zkey], r[zkey])
            for key in keys:
                bad[key] = np.exp(good[zkey] - z) * good[key] + np.exp(r[zkey] - z) * r[key]
        gr_bad = kt.gr_of(rows[:k] + [bad] + rows[k + 1:], len(x))
        hidden = np.allclose(gr_bad, gr_ref, **tc.GR_TOL) and np.abs(gr_bad - gr_ref).max() > 0
        err = max(tc.count_error(bad[key], good[key]).max() for key in tc.COUNTS)
        if hidden and err > 10 * tc.ROW_RTOL and (found is None or err > found[0]):
            found = (err, db, bad, gr_bad)
    assert found is not None
    err, db, bad, gr_bad = found
    np.testing.assert_allclose(gr_bad, gr_ref, **tc.GR_TOL)               # the hole: invisible to the batch gradient
    counts = {key: np.array([bad[key] if j == k else r[key] for j, r in enumerate(rows)]) for key in tc.COUNTS}
    stats = np.array([[r["Zo"], r["Zari"], r["Znasi"], r["f"], r["skipped"]] for r in rows])
    refs_t = kt.train_refs(rows, len(x))
    with pytest.raises(AssertionError, match=r"sequence %d \(L 16, with motif\): E[NH][ox]\[\d+\]" % k):
        tc.check_rows(stats, counts, refs_t, seqs, quals)
    for key in tc.COUNTS:
        counts[key][k] = good[key]
    tc.check_rows(stats, counts, refs_t, seqs, quals)                     # (and the unperturbed rows pass)
