// node_mea_rules.h -- maximum expected accuracy motif alignments and site lists, host / device.
//
// A node row of length L (0 = 'z' .. M-1 = 'o', the numbering of psihat) is valid if it is the row of some alignment: all 'z', or
// z^a n1^r1 .. nk^rk o^c over the inner nodes in order, r >= 1 (r >= 0 for a '*' node), the body not empty.  As a chain over the
// positions: row[p+1] == row[p], or row[p+1] > row[p] with only '*' nodes strictly between them, never 0 -> M-1; the first entry
// is 0 or an inner node with only '*' nodes before it; the last entry is 0, M-1, or an inner node with only '*' nodes behind it.
// The predecessors of a node are therefore one range lo(m) .. m, and the lists are three ints per node.
//
// With N the node profile of node_rules.h (clamped) and g(m) = gamma on the inner nodes, 1 on 'z' and 'o',
//     score(row) = sum_p g(row[p]) N(p, row[p])
//     V(0, m) = g(m) N(0, m) for a first node,   V(p, m) = g(m) N(p, m) + max over lo(m) <= m' <= m of V(p-1, m')
// and the best row ends in the last node of greatest V(L-1, .).  Slot 0 of a sequence is that row; the positions that carry its
// inner nodes are one contiguous region, site 0.  Slot k is the best row that puts no inner node on a position of the sites
// 0 .. k-1 (V = -inf there; 'z' and 'o' stay allowed); the list ends at the first slot whose best row is all 'z'.
//
// Ties: the lower predecessor at every step, the lower final node (a strict > over ascending candidates), so the result is a
// function of the profile's bits.  The row maximises a sum of marginals and need not be a derivation of positive probability.
//
// One rule for the kernel (node_mea_kernels.hip: the lanes over the nodes) and the test-only CPU driver (tests/node_mea_emul.cpp).
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>

#include "dp_rules.h"

namespace elemdp {

constexpr int kNodeMeaMaxSites = 64;   // most sites of a sequence a call may ask for
constexpr int kNodeMeaMaxNodes = 255;  // the node bytes

struct NodeMeaLists {
  const int32_t* v;   // lo[M], first[M], last[M]
  int32_t M;
  ELEMDP_HD int lo(int m) const { return v[m]; }                     // predecessors of m: lo(m) .. m
  ELEMDP_HD bool first(int m) const { return v[M + m] != 0; }        // m may start a row
  ELEMDP_HD bool last(int m) const { return v[2 * M + m] != 0; }     // m may end a row
  ELEMDP_HD bool inner(int m) const { return m > 0 && m < M - 1; }
};

// the blob NodeMeaLists reads, from the node names 'z' .. 'o' of the automaton (host)
inline void node_mea_lists_build(const char* names, int M, std::vector<int32_t>* blob) {
  blob->assign((size_t)3 * M, 0);
  int32_t* lo = blob->data();
  int32_t* first = lo + M;
  int32_t* last = lo + 2 * M;
  for (int m = 1; m < M; ++m) {
    int k = m - 1;
    while (k > 0 && names[k] == '*') --k;   // (the nearest node below m that a row cannot skip, or 'z')
    lo[m] = k;
  }
  if (M >= 2 && lo[M - 1] == 0) lo[M - 1] = 1;   // (never 'z' -> 'o': the body is not empty)
  first[0] = 1;
  for (int m = 1; m < M - 1; ++m) first[m] = lo[m] == 0;
  last[0] = 1;
  if (M >= 2) last[M - 1] = 1;
  for (int m = M - 2; m >= 1; --m) {
    last[m] = 1;
    if (names[m] != '*') break;   // (nothing below a node that must occur may end the row)
  }
}

ELEMDP_HD double node_mea_neg_inf() { return -HUGE_VAL; }
ELEMDP_HD double node_mea_gain(const NodeMeaLists& nl, double gamma, int m) { return nl.inner(m) ? gamma : 1.; }

// does position p lie in one of the sites [s0[j], s1[j]), j < k?
ELEMDP_HD bool node_mea_barred(const int32_t* s0, const int32_t* s1, int k, int p) {
  for (int j = 0; j < k; ++j)
    if (s0[j] <= p && p < s1[j]) return true;
  return false;
}

// V(0, m); row = N(0, .); barred: position 0 lies in an earlier site
ELEMDP_HD double node_mea_first(const NodeMeaLists& nl, double gamma, const double* row, int m, bool barred) {
  if (!nl.first(m) || (barred && nl.inner(m))) return node_mea_neg_inf();
  return node_mea_gain(nl, gamma, m) * row[m];
}

// V(p, m), p >= 1, from prev = V(p-1, .) and row = N(p, .); *from = the predecessor taken (the lowest of the greatest)
ELEMDP_HD double node_mea_step(const NodeMeaLists& nl, double gamma, const double* row, const double* prev, int m, bool barred, int* from) {
  int arg = nl.lo(m);
  double best = prev[arg];
  for (int k = arg + 1; k <= m; ++k) {
    const double v = prev[k];
    if (v > best) { best = v; arg = k; }
  }
  *from = arg;
  if (barred && nl.inner(m)) return node_mea_neg_inf();
  return node_mea_gain(nl, gamma, m) * row[m] + best;
}

// the final node: the lowest last node of greatest V(L-1, .) (V(L-1, 0), the row of 'z' alone, is always finite)
ELEMDP_HD int node_mea_final(const NodeMeaLists& nl, const double* V, double* score) {
  int arg = 0;
  double best = V[0];
  for (int m = 1; m < nl.M; ++m)
    if (nl.last(m) && V[m] > best) { best = V[m]; arg = m; }
  *score = best;
  return arg;
}

struct NodeMeaSite {
  int32_t start, end;   // the positions [start, end) carry the inner nodes; -1, -1 without any
  double score, conf;   // score of the whole row; mean of N(p, row[p]) over the site
};
ELEMDP_HD NodeMeaSite node_mea_no_site() { return NodeMeaSite{-1, -1, __builtin_nan(""), __builtin_nan("")}; }

// the row that ends in `fin`, from the backpointers bp[M p + m] (p >= 1), and its site; prof = N of the sequence
ELEMDP_HD NodeMeaSite node_mea_trace(const NodeMeaLists& nl, int L, const double* prof, const uint8_t* bp, int fin, double score,
                                     uint8_t* row) {
  const int M = nl.M;
  NodeMeaSite s{-1, -1, score, 0.};
  int m = fin;
  for (int p = L - 1; p >= 0; --p) {
    row[p] = (uint8_t)m;
    if (nl.inner(m)) {
      if (s.end < 0) s.end = p + 1;
      s.start = p;
      s.conf += prof[(size_t)M * p + m];
    }
    if (p > 0) m = bp[(size_t)M * p + m];
  }
  s.conf = s.end < 0 ? __builtin_nan("") : s.conf / (double)(s.end - s.start);
  return s;
}

}  // namespace elemdp
