// joint_rules.h -- joint node-by-context posteriors and the emission counts behind a motif logo, host / device.
//
// J(p, m, c): the probability that base p of a sequence is emitted by pattern node m (0 = 'z' .. M-1 = 'o') AND carries the
// structure letter c (O L R H B I M, CtxCol order), over the ensemble of the scan's first sum pass (terminals ari and nasi,
// Z = Z(ari, nasi): the ensemble of pair_rules.h, ctx_rules.h and node_rules.h).  Five columns are the parts of node_rules.h
// routed by letter instead of summed (the parts option node_rules separates):
//
//   O  rule 8                       L  the left base of 1a / 1b             R  the right base of 1a / 1b
//   M  3a + 5a (in the compact form with the pair-table part, NodeLin::chain)
//
// The L <- L emissions split into H, B and I.  The outside L entry is linear in its seeds (lin_outside_target_u:
// oL = t6b + sL + HL; loop_outside_entry): the hairpin seed of rule 6b, the seeds of the rule-6c items, and the chain from the
// row's next entry.  For kind c in {H, B}, a loop state s and a cell (i, d), d >= 1, with in(L, i, d, s) live:
//
//   G_c(i, d, s) = seed_c(i, d, s) + sum over the loop states par with a right transition par -> s:
//                                        G_c(i, d + 1, par) w_emit(par, tf, i + d)            under i + d < L, d + 1 <= W
//   seed_H(i, d, s) = out(E, i, d, s) w_hairpin(s, cell(i - 1, d + 2))                         under e_ok(i, d)        (rule 6b)
//   seed_B(i, d, s) = sum over the rule-6c items with [i, i + d) as their only non-empty run, found as ctx_cell finds them (the
//                     run's by-left list with l == j, its by-right list with k == i, both under item_in; tuples quad2 / quad3
//                     of s; weights from tsc):  out(E, outer, par) in(P, inner, s1) in(L, empty run, s') w_item(par)
//   G_c = 0 where in(L, i, d, s) is dead, as the outside L entry is.
//
//   J(p, m, c) = sum_i sum_{s loop, st_r(s) = m, in(L, i, d, s) live} in(L, i, d, s) G_c(i, d, s) / Z,        d = p + 1 - i
//   J(p, m, I) = max(0, [the L <- L part of N(p, m)] - J(p, m, H) - J(p, m, B))
//
// seed_B is the b term of ctx_cell kept per state of the run and without the in(L) factor of the run itself; the chain carries
// the guards and weights of the L <- L line of lin_outside_target_u / loop_outside_chain.  Every entry is clamped to [0, 1];
// nothing is renormalised.  sum_c J(p, m, c) = N(p, m) of node_rules.h, and sum_m J(p, m, c) = the profile of ctx_rules.h
// wherever the tables' inside and outside agree (with max_iloop < 30 the I and M columns follow the tables: SURVEY §7 quirk ii).
// A sequence without any parse has J(p, 0, O) = 1 and 0 elsewhere.  Without secondary structure (ELEMDP_NO_RSS) only rule 8
// exists and the band tables are not read.
//
// Is out(E) stored wherever the seeds read it?  Yes.  k4_out<OUT_SCAN> stores out(E) at every cell where e_ok holds, for every
// state with a column in plane E, in both `fast` forms (fast_outside_unary: `if (eok && cEo >= 0) out.band[..ST_E..] = oE`;
// lin_outside_target_u: `out.st(ST_E, d, i, s, oE, eok)`), the value being 0 where in(E) is.  seed_H reads out(E, i, d, s) under
// e_ok(i, d); seed_B reads out(E) of an item's outer cell, which is an E cell by the plan (the enumeration of the inside pass:
// item_in) -- the very reads ctx_cell makes.  A state without a column reads as 0 through TableView::ld.
//
// The per-cell sums in(L) G_c / Z are kept by emitted node, over the nodes that loop states can emit (JointLists::slot), never
// by state: X[((i (W + 1) + d) 2 + kind) n_slots + slot].  Counts: counts[m][c][b] = sum_p J(p, m, c) [seq[p] = b], b = 0 .. 4
// (N A C G U), positions in increasing order.  One rule for both forms (JointLin / JointLog).  Liveness is decided before every
// load, by control flow, never by a multiply.
#pragma once
#include <vector>

#include "node_rules.h"

namespace elemdp {

constexpr int kJointBases = 5;   // N A C G U
enum JointKind : int { JK_H = 0, JK_B = 1, JK_KINDS = 2 };
// the terms of G as bits of JointLists::parts (every bit in the product; the CPU driver of the tests drops one to show that
// its references see each term)
enum JointPart : int { JP_SEED_H = 1, JP_SEED_B = 2, JP_CHAIN = 4, JP_ALL = 7 };

struct JointLists {
  NodeLists nl;          // (rules is not read here: the five routed parts take their rule bits one at a time)
  const int32_t* slot;   // M entries: the scratch slot of a node that loop states can emit, -1 for the others
  int32_t n_slots;
  int32_t parts;         // JointPart bits
};

// the blob of node_lists_build followed by the slot map; returns the number of slots.  *slot_at: where the map starts.
inline int joint_lists_build(const AutomatonLayout& A, const int32_t* I, std::vector<int32_t>* blob, size_t* slot_at) {
  node_lists_build(A, I, blob);
  std::vector<int32_t> slot(A.M, -1);
  int n = 0;
  for (int node = 0; node < A.M; ++node)   // (the offsets of list NK_L: NodeLists::begin / end)
    if ((*blob)[NK_L * (A.M + 1) + node + 1] > (*blob)[NK_L * (A.M + 1) + node]) slot[node] = n++;
  *slot_at = blob->size();
  blob->insert(blob->end(), slot.begin(), slot.end());
  return n;
}

struct JointLin : NodeLin {
  ELEMDP_HD explicit JointLin(double invZ_) : NodeLin(invZ_) {}
  ELEMDP_HD double zero() const { return 0.; }
  ELEMDP_HD double add(double a, double b) const { return a + b; }
};
struct JointLog : NodeLog {
  ELEMDP_HD explicit JointLog(double lnZ_) : NodeLog(lnZ_) {}
  ELEMDP_HD double zero() const { return ELEMDP_NEG_INF; }
  ELEMDP_HD double add(double a, double b) const { return lse2(a, b); }
};

ELEMDP_HD size_t joint_cell_at(const SeqView& q, int n_slots, int i, int d, int kind) {
  return (((size_t)i * (q.W + 1) + d) * JK_KINDS + kind) * (size_t)n_slots;
}
// doubles of the per-cell scratch of one table slot (host)
inline size_t joint_scratch_size(int Lmax, int Wmax, int n_slots) {
  return ((size_t)Lmax + 1) * ((size_t)Wmax + 1) * JK_KINDS * (size_t)(n_slots > 0 ? n_slots : 1);
}

// seed_B of loop state s at the run [i, i + d): the items of the by-left list, then of the by-right list, in list order; the
// filter does not depend on the state, so lanes that take the states of one run walk the lists together
template <class F>
ELEMDP_HD double joint_seed_b(const F& f, const ModelView& m, const SeqView& q, const TableView& in, const TableView& out, int d, int i,
                              int s) {
  const AutomatonLayout& A = m.lay;
  const int32_t* G = m.big;
  double a = f.zero();
  const int lc = q.cell(i, d);
  for (int n = q.by_left_off[lc]; n < q.by_left_off[lc + 1]; ++n) {          // left run of a bulge: the right run L(l, j) is empty
    const int idx = q.by_left_idx[n];
    const LoopItem it = q.items[idx];
    if (it.l != it.j || !q.item_in[idx]) continue;
    const double w0 = f.w_item(m, 0, it.tsc), w1 = f.w_item(m, 1, it.tsc);
    for (int u = G[A.quad2_off + s]; u < G[A.quad2_off + s + 1]; ++u) {
      const int par = G[A.quad2_ent + 3 * u], s1 = G[A.quad2_ent + 3 * u + 1], s3 = G[A.quad2_ent + 3 * u + 2];
      a = f.add(a, f.mul(f.ld(out, ST_E, it.j - it.i, it.i, par),
                         f.mul(f.ld(in, ST_P, it.l - it.k, it.k, s1), f.mul(f.ld(in, ST_L, 0, it.j, s3), lamk(m, par) ? w1 : w0))));
    }
  }
  for (int n = q.by_right_off[lc]; n < q.by_right_off[lc + 1]; ++n) {        // right run of a bulge: the left run L(i, k) is empty
    const int idx = q.by_right_idx[n];
    const LoopItem it = q.items[idx];
    if (it.k != it.i || !q.item_in[idx]) continue;
    const double w0 = f.w_item(m, 0, it.tsc), w1 = f.w_item(m, 1, it.tsc);
    for (int u = G[A.quad3_off + s]; u < G[A.quad3_off + s + 1]; ++u) {
      const int par = G[A.quad3_ent + 3 * u], s1 = G[A.quad3_ent + 3 * u + 1], s2 = G[A.quad3_ent + 3 * u + 2];
      a = f.add(a, f.mul(f.ld(out, ST_E, it.j - it.i, it.i, par),
                         f.mul(f.ld(in, ST_P, it.l - it.k, it.k, s1), f.mul(f.ld(in, ST_L, 0, it.i, s2), lamk(m, par) ? w1 : w0))));
    }
  }
  return a;
}

// G_H and G_B of loop state s at the cell (i, d), d >= 1, i + d <= L, whose in(L, i, d, s) is live (the caller checked).
// ph / pb: G_H / G_B of the cell (i, d + 1) by state (zero() where in(L) is dead there), or null where that cell does not exist.
struct JointG { double h, b; };
template <class F>
ELEMDP_HD JointG joint_entry(const F& f, const JointLists& jl, const ModelView& m, const SeqView& q, const TableView& in,
                             const TableView& out, int d, int i, int s, const double* ph, const double* pb) {
  const AutomatonLayout& A = m.lay;
  const int32_t* I = m.ints;
  JointG g{f.zero(), f.zero()};
  if ((jl.parts & JP_SEED_H) && q.e_ok(i, d))
    g.h = f.mul(f.ld(out, ST_E, d, i, s), f.w_hairpin(m, q, s, q.cell(i - 1, d + 2)));
  if (jl.parts & JP_SEED_B) g.b = joint_seed_b(f, m, q, in, out, d, i, s);
  const int j = i + d;
  if ((jl.parts & JP_CHAIN) && ph && j < q.L && d + 1 <= q.W)
    for (int t = I[A.rright_off + s]; t < I[A.rright_off + s + 1]; ++t) {
      const int par = I[A.rright_ent + 2 * t];
      if (!I[A.st_is_loop + par]) continue;
      const double gh = ph[par], gb = pb[par];
      if (f.dead(gh) && f.dead(gb)) continue;
      const double w = f.w_emit(m, q, par, I[A.rright_ent + 2 * t + 1], j);
      if (!f.dead(gh)) g.h = f.add(g.h, f.mul(gh, w));
      if (!f.dead(gb)) g.b = f.add(g.b, f.mul(gb, w));
    }
  return g;
}

// in(L) G / Z of one cell summed over the loop states that emit `node`, states in list order.  inL, g: by state.
template <class F>
ELEMDP_HD double joint_node_sum(const F& f, const NodeLists& nl, int node, const double* inL, const double* g) {
  double a = 0.;
  for (int e = nl.begin(NK_L, node); e < nl.end(NK_L, node); ++e) {
    const int s = nl.ent(e)[0];
    if (f.dead(inL[s]) || f.dead(g[s])) continue;
    a += f.post(f.mul(inL[s], g[s]));
  }
  return a;
}

// one row of a sequence, serial (the CPU driver, the log-space form): d from min(W, L - i) down to 1.  vec: 5 S doubles.
// X: the per-cell scratch of the sequence.
template <class F>
ELEMDP_HD void joint_row(const F& f, const JointLists& jl, const ModelView& m, const SeqView& q, const TableView& in, const TableView& out,
                         int i, double* vec, double* X) {
  const AutomatonLayout& A = m.lay;
  const int32_t* I = m.ints;
  const int S = A.S, M = jl.nl.M;
  double* inL = vec;
  double* cur[2] = {vec + S, vec + 2 * S};
  double* prev[2] = {vec + 3 * S, vec + 4 * S};
  const int dmax = q.L - i < q.W ? q.L - i : q.W;
  for (int d = dmax; d >= 1; --d) {
    for (int s = 0; s < S; ++s) {
      JointG g{f.zero(), f.zero()};
      double v = f.zero();
      if (I[A.st_is_loop + s]) {
        v = f.ld(in, ST_L, d, i, s);
        if (!f.dead(v)) g = joint_entry(f, jl, m, q, in, out, d, i, s, d < dmax ? prev[0] : nullptr, d < dmax ? prev[1] : nullptr);
      }
      inL[s] = v; cur[0][s] = g.h; cur[1][s] = g.b;
    }
    for (int node = 0; node < M; ++node) {
      const int k = jl.slot[node];
      if (k < 0) continue;
      X[joint_cell_at(q, jl.n_slots, i, d, JK_H) + k] = joint_node_sum(f, jl.nl, node, inL, cur[0]);
      X[joint_cell_at(q, jl.n_slots, i, d, JK_B) + k] = joint_node_sum(f, jl.nl, node, inL, cur[1]);
    }
    for (int k = 0; k < 2; ++k) { double* t = cur[k]; cur[k] = prev[k]; prev[k] = t; }
  }
}

// the cells (p + 1 - d, d) of position p dealt to `part` of `nparts` by d: their stored sums of `kind` in slot k
ELEMDP_HD double joint_gather_part(const double* X, const SeqView& q, int n_slots, int p, int k, int kind, int part, int nparts) {
  double a = 0.;
  for (int d = 1 + part; d <= q.W && d <= p + 1; d += nparts) a += X[joint_cell_at(q, n_slots, p + 1 - d, d, kind) + k];
  return a;
}

// the five routed parts of node_rules.h at position p for `node`, the cells dealt as node_cells_part deals them
struct JointParts { double l, r, u, mm; };
template <class F>
ELEMDP_HD JointParts joint_cells_part(const F& f, const NodeLists& nl0, const ModelView& m, const SeqView& q, const TableView& in,
                                      const TableView& out, int p, int node, int part, int nparts) {
  NodeLists nl = nl0;
  JointParts r{0., 0., 0., 0.};
  for (int d = 1 + part; d <= q.W; d += nparts) {
    if (d <= p + 1) {
      const int i = p + 1 - d;
      nl.rules = NR_LOOP;   r.u += node_cell_right(f, nl, m, q, in, out, d, i, node);
      nl.rules = NR_3A;     r.mm += node_cell_right(f, nl, m, q, in, out, d, i, node);
      nl.rules = NR_PAIR_R; r.r += node_cell_right(f, nl, m, q, in, out, d, i, node);
    }
    if (p + d <= q.L) {
      nl.rules = NR_5A;     r.mm += node_cell_left(f, nl, m, q, in, out, d, p, node);
      nl.rules = NR_PAIR_L; r.l += node_cell_left(f, nl, m, q, in, out, d, p, node);
    }
  }
  return r;
}
template <class F>
ELEMDP_HD double joint_exterior(const F& f, const NodeLists& nl0, const ModelView& m, const SeqView& q, const TableView& in,
                                const TableView& out, int p, int node) {
  NodeLists nl = nl0;
  nl.rules = NR_EXT;
  return node_exterior(f, nl, m, q, in, out, p, node);
}

// one (position, node): the 7 letters from the sums of the parts
ELEMDP_HD void joint_compose(double o, const JointParts& c, double h, double b, double* row) {
  h = ctx_clamp(h);
  b = ctx_clamp(b);
  row[CTX_O] = ctx_clamp(o); row[CTX_L] = ctx_clamp(c.l); row[CTX_R] = ctx_clamp(c.r);
  row[CTX_H] = h; row[CTX_B] = b;
  row[CTX_I] = ctx_clamp(c.u - h - b);
  row[CTX_M] = ctx_clamp(c.mm);
}
ELEMDP_HD void joint_no_parse(int node, double* row) {
  row[CTX_O] = node == 0 ? 1. : 0.;
  for (int c = 1; c < CTX_COLS; ++c) row[c] = 0.;
}

// J(p, node, .), serial (the CPU driver, the log-space form); cells false: a model without secondary structure (X is not read)
template <class F>
ELEMDP_HD void joint_value(const F& f, const JointLists& jl, const ModelView& m, const SeqView& q, const TableView& in,
                           const TableView& out, const double* X, int p, int node, bool cells, double* row) {
  JointParts c{0., 0., 0., 0.};
  double h = 0., b = 0.;
  if (cells) {
    c = joint_cells_part(f, jl.nl, m, q, in, out, p, node, 0, 1);
    const int k = jl.slot[node];
    if (k >= 0) {
      h = joint_gather_part(X, q, jl.n_slots, p, k, JK_H, 0, 1);
      b = joint_gather_part(X, q, jl.n_slots, p, k, JK_B, 0, 1);
    }
  }
  joint_compose(joint_exterior(f, jl.nl, m, q, in, out, p, node), c, h, b, row);
}

// counts[(m 7 + c) 5 + b] of one sequence for entry t = (m 7 + c) 5 + b: positions in increasing order
ELEMDP_HD double joint_count(const double* profile, const uint8_t* seq, int L, int M, int t) {
  const int b = t % kJointBases, mc = t / kJointBases;
  double a = 0.;
  for (int p = 0; p < L; ++p)
    if (seq[p] == b) a += profile[(size_t)CTX_COLS * M * p + mc];
  return a;
}

}  // namespace elemdp
