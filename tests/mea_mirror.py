"""Host mirror of the maximum expected accuracy rule (rnaelem_amd/csrc/mea_rules.h).

Same table, candidate order and sums as the kernel: every candidate list is [unpaired, e = 2, 3, ...], the first greatest wins
(np.argmax) -- a later candidate replaces the current one only if it is strictly greater --, the pair weight is rounded before
any sum, w = (2 gamma) * P, and a pair candidate is (w(i, e) + M(i+1, e-2)) + rest.  Vectorised over e (and over i for a diagonal
of M), so the GPU result can be compared with it bit for bit."""
import numpy as np


def mea_fold(P, kept, q, gamma):
    """P, kept: [i][d] arrays of shape (L+1, W+1) (cell (i, d): bases i and i+d-1 pair); q: the L unpaired probabilities.
    -> (structure, score)"""
    q = np.asarray(q, dtype=np.float64)
    L = len(q)
    W = P.shape[1] - 1
    w = (2.0 * gamma) * np.asarray(P, dtype=np.float64)
    kept = np.asarray(kept, dtype=bool)
    M = np.zeros((L + 1, W + 1))
    chM = np.zeros((L + 1, W + 1), dtype=np.int64)
    for d in range(1, min(W, L) + 1):
        i = np.arange(0, L - d + 1)
        cand = np.full((len(i), d), -np.inf)
        cand[:, 0] = M[i + 1, d - 1] + q[i]
        if d >= 2:
            e = np.arange(2, d + 1)
            I, E = i[:, None], e[None, :]
            v = (w[I, E] + M[I + 1, E - 2]) + M[I + E, d - E]
            cand[:, 1:] = np.where(kept[I, E], v, -np.inf)
        k = np.argmax(cand, axis=1)
        M[i, d] = cand[np.arange(len(i)), k]
        chM[i, d] = np.where(k == 0, 0, k + 1)
    F = np.zeros(L + 1)
    chF = np.zeros(L + 1, dtype=np.int64)
    for i in range(L - 1, -1, -1):
        emax = min(W, L - i)
        cand = np.full(max(emax, 1), -np.inf)
        cand[0] = F[i + 1] + q[i]
        if emax >= 2:
            e = np.arange(2, emax + 1)
            v = (w[i, e] + M[i + 1, e - 2]) + F[i + e]
            cand[1:] = np.where(kept[i, e], v, -np.inf)
        k = int(np.argmax(cand))
        F[i] = cand[k]
        chF[i] = 0 if k == 0 else k + 1
    s = ["."] * L
    i = 0
    while i < L:
        e = int(chF[i])
        if e == 0:
            i += 1
            continue
        s[i], s[i + e - 1] = "(", ")"
        stack = [(i + 1, e - 2)]
        while stack:
            a, d = stack.pop()
            while d > 0:
                c = int(chM[a, d])
                if c == 0:
                    a, d = a + 1, d - 1
                    continue
                s[a], s[a + c - 1] = "(", ")"
                stack.append((a + 1, c - 2))
                a, d = a + c, d - c
        i += e
    return "".join(s), float(F[0])


def pairs_of(structure):
    """-> list of cells (i, d) of a dot-bracket string (bases i and i+d-1 pair)"""
    out, st = [], []
    for k, c in enumerate(structure):
        if c == "(":
            st.append(k)
        elif c == ")":
            i = st.pop()
            out.append((i, k - i + 1))
        else:
            assert c == ".", c
    assert not st
    return sorted(out)


def expected_accuracy(structure, P, q, gamma):
    """the objective of a structure, summed in position order (not the fold's order)"""
    cells = pairs_of(structure)
    paired = np.zeros(len(q), dtype=bool)
    tot = 0.0
    for i, d in cells:
        tot += (2.0 * gamma) * P[i, d]
        paired[i] = paired[i + d - 1] = True
    return tot + float(np.sum(np.asarray(q)[~paired]))


def pair_matrix(L, W, ii, jj, pp):
    """the [i][d] P array and kept mask of one sequence from a pair list (cells (i, j = i + d))"""
    P = np.zeros((L + 1, W + 1))
    kept = np.zeros((L + 1, W + 1), dtype=bool)
    d = np.asarray(jj) - np.asarray(ii)
    P[ii, d] = pp
    kept[ii, d] = True
    return P, kept
