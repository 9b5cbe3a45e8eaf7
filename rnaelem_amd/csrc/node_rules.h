// node_rules.h -- posterior motif-node profiles under the motif model, host / device.
//
// N(p, m): the probability that base p of a sequence is emitted by pattern node m (0 = 'z' .. M-1 = 'o', the numbering of psihat and
// of the sampler's node bytes), over the ensemble of the scan's first sum pass (terminals ari and nasi, Z = Z(ari, nasi): the
// ensemble of pair_rules.h and ctx_rules.h), from its inside and outside tables.  A derivation emits every base exactly once, by
// one of five emitting rules; the node is the one sample_walk / trace_back write.  Cell [i, j), d = j - i; every product below
// is divided by Z; guards and liveness are those of lin_inside_target_u:
//
//   L <- L      in(L, i, d, s) out(L, i, d, s)                                       d >= 1, s a loop state      st_r(s) at j-1
//               (every L entry with d >= 1 is made by one right emission of its own r-node at j-1)
//   3a  2 <- 2  out(2, i, d, s) wr(s, tf, j-1) in(2, i, d-1, s1)                     s1 in right(s), under do2   st_r(s) at j-1
//   5a  M <- M  out(M, i, d, s) wl(sl, tf, i) in(M, i+1, d-1, sl)                    sl in left(s), under doM    st_l(sl) at i
//   1a / 1b     out(P, i, d, s) wp(s, sp, tf, i, j-1) (in(P, i+1, d-2, sp) xst + in(E, i+1, d-2, sp))
//                                                                                    sp in pair(s), under pok, cE, cP
//                                                                                    st_l(sp) at i and st_r(s) at j-1
//   8   O <- O  out_o(p+1, s) wt in_o(p, s1)                                         s1 in right(s), under unp[p]  st_r(s) at p
//
// The compact scaled-linear tables keep only the direct part of out(2) (rules 4a and 3a: lin_outside_target_u); what a 2 entry
// takes as the right part of a bifurcation lives in the pair table of the factorised rule 2, whose tail step IS rule 3a there
// (lin_inside_apair / lin_outside_apair).  So that form adds
//       out_A(i, d, p) wr(t(p), tf, j-1) in_A(i, d-1, pc)                            pc in chain(p), entries of (i, d-1) exist
//                                                                                    st_r(t(p)) at j-1
// which summed over the split points is exactly the missing part of out(2) times the same emission.  The dense log-space tables
// hold the whole out(2) and have no pair table.
//
// N(p, m) is the sum of these posteriors routed to (p, m), clamped to [0, 1]: no remainder column, no renormalisation.  A row sums
// to 1 wherever the tables' inside and outside agree (with max_iloop < 30 the outside pass enumerates interior loops the inside
// pass does not, SURVEY §7 quirk ii, and the sum follows the tables).  A sequence without any parse has N(p, 0) = 1 and 0
// elsewhere.  Without secondary structure (ELEMDP_NO_RSS) only rule 8 exists: the cell part is skipped, the tables of the band are
// not read.
//
// The transitions are grouped by the node they emit (NodeLists, built on the host from the flattened automaton): the result of one
// (position, node) is a gather over the cells whose right base is p (L, 3a, the pair's right base), the cells whose left base is p
// (5a, the pair's left base) and rule 8.  One rule for both forms (NodeLin / NodeLog), as CtxLin / CtxLog.  Liveness is decided
// before every load, by control flow, never by a multiply.
#pragma once
#include <vector>

#include "ctx_rules.h"

namespace elemdp {

// lists of the emitting transitions by emitted node; 3 ints per entry
enum NodeKind : int {
  NK_L = 0,    // (s, -, -)      loop state s, by st_r(s)
  NK_R = 1,    // (s, s1, tf)    right transition s -> s1 (rules 3a, 8), by st_r(s)
  NK_A = 2,    // (p, pc, tf)    tail step of the factorised rule 2 from pair pc to pair p, by st_r(t(p))
  NK_PR = 3,   // (s, sp, tf)    pair transition s -> sp, by st_r(s): its right base
  NK_PL = 4,   // (s, sp, tf)    the same transitions by st_l(sp): their left base
  NK_M = 5,    // (s, sl, tf)    left transition s -> sl (rule 5a), by st_l(sl)
  NK_KINDS = 6
};
// the rules of the header as bits of NodeLists::rules (engine option node_rules; every bit by default).  A subset gives that part
// of the profile: the L <- L part is U = H + B + I of ctx_rules.h, the left / right bases of rules 1a / 1b its L / R, the rule-8 part
// its O, rules 3a and 5a together its M.
enum NodeRule : int { NR_LOOP = 1, NR_3A = 2, NR_5A = 4, NR_PAIR_L = 8, NR_EXT = 16, NR_PAIR_R = 32, NR_ALL = 63 };
struct NodeLists {
  const int32_t* v;   // NK_KINDS * (M + 1) offsets (entry indices), then the entries
  int32_t M;
  int32_t rules;      // NodeRule bits
  ELEMDP_HD int begin(int kind, int node) const { return v[kind * (M + 1) + node]; }
  ELEMDP_HD int end(int kind, int node) const { return v[kind * (M + 1) + node + 1]; }
  ELEMDP_HD const int32_t* ent(int e) const { return v + NK_KINDS * (M + 1) + 3 * e; }
};

// the blob NodeLists reads, from a flattened automaton (host).  Within a node the entries keep the order of the automaton's lists.
inline void node_lists_build(const AutomatonLayout& A, const int32_t* I, std::vector<int32_t>* blob) {
  const int M = A.M;
  struct Ent { int node, a, b, tf; };
  std::vector<Ent> kinds[NK_KINDS];
  for (int s = 0; s < A.S; ++s) {
    const int sr = I[A.st_r + s];
    if (I[A.st_is_loop + s]) kinds[NK_L].push_back({sr, s, 0, 0});
    for (int t = I[A.right_off + s]; t < I[A.right_off + s + 1]; ++t)
      kinds[NK_R].push_back({sr, s, I[A.right_ent + 2 * t], I[A.right_ent + 2 * t + 1]});
    for (int t = I[A.pair_off + s]; t < I[A.pair_off + s + 1]; ++t) {
      const int sp = I[A.pair_ent + 2 * t], tf = I[A.pair_ent + 2 * t + 1];
      kinds[NK_PR].push_back({sr, s, sp, tf});
      kinds[NK_PL].push_back({I[A.st_l + sp], s, sp, tf});
    }
    for (int t = I[A.left_off + s]; t < I[A.left_off + s + 1]; ++t) {
      const int sl = I[A.left_ent + 2 * t];
      kinds[NK_M].push_back({I[A.st_l + sl], s, sl, I[A.left_ent + 2 * t + 1]});
    }
  }
  for (int p = 0; p < A.n_ap; ++p)
    for (int e = I[A.ap_chain_off + p]; e < I[A.ap_chain_off + p + 1]; ++e)
      kinds[NK_A].push_back({I[A.st_r + I[A.ap_t + p]], p, I[A.ap_chain_ent + 2 * e], I[A.ap_chain_ent + 2 * e + 1]});
  blob->assign((size_t)NK_KINDS * (M + 1), 0);
  int n = 0;
  for (int k = 0; k < NK_KINDS; ++k) {
    for (int node = 0; node < M; ++node) {
      (*blob)[k * (M + 1) + node] = n;
      for (const Ent& e : kinds[k])
        if (e.node == node) { blob->push_back(e.a); blob->push_back(e.b); blob->push_back(e.tf); ++n; }
    }
    (*blob)[k * (M + 1) + M] = n;
  }
}

struct NodeLin : CtxLin {
  ELEMDP_HD explicit NodeLin(double invZ_) : CtxLin{invZ_} {}
  ELEMDP_HD double w_left(const ModelView& m, const SeqView& q, int ch, int tf, int pos) const { return lw_left(m, q, ch, tf, pos); }
  ELEMDP_HD double w_pair2(const ModelView& m, const SeqView& q, int par, int ch, int tf, int pi, int pj) const { return lw_pair(m, q, par, ch, tf, pi, pj); }
  ELEMDP_HD double w_stack(const ModelView& m, const SeqView& q, int s, int c) const { return xw_cell(q, lamk(m, s), XT_STACK, c); }
  // the tail steps of the pair table at cell (i, d) that emit `node`; the entries of (i, d-1) and (i, d) exist (the caller checked)
  ELEMDP_HD double chain(const NodeLists& nl, const ModelView& m, const SeqView& q, const TableView& in, const TableView& out, int d,
                         int i, int node) const {
    double a = 0.;
    for (int e = nl.begin(NK_A, node); e < nl.end(NK_A, node); ++e) {
      const int32_t* t = nl.ent(e);
      const double o = out.a(d, i, t[0]);
      if (o == 0.) continue;
      a += post(o * (in.a(d - 1, i, t[1]) * lw_right(m, q, m.ints[m.lay.ap_t + t[0]], t[2], i + d - 1)));
    }
    return a;
  }
};
struct NodeLog : CtxLog {
  ELEMDP_HD explicit NodeLog(double lnZ_) : CtxLog{lnZ_} {}
  ELEMDP_HD double w_left(const ModelView& m, const SeqView& q, int ch, int tf, int pos) const { return elemdp::w_left(m, q, ch, tf, pos); }
  ELEMDP_HD double w_pair2(const ModelView& m, const SeqView& q, int par, int ch, int tf, int pi, int pj) const { return w_pair(m, q, par, ch, tf, pi, pj); }
  ELEMDP_HD double w_stack(const ModelView& m, const SeqView& q, int s, int c) const {
    const double e = q.e_stack[c];
    return e == ELEMDP_NEG_INF ? ELEMDP_NEG_INF : m.lam(s) * e;
  }
  ELEMDP_HD double chain(const NodeLists&, const ModelView&, const SeqView&, const TableView&, const TableView&, int, int, int) const {
    return 0.;   // (the dense out(2) is whole)
  }
};

// posterior of the pair transitions of list `kind` (NK_PR / NK_PL) at the kept cell (i, d) that emit `node`
template <class F>
ELEMDP_HD double node_pairs(const F& f, const NodeLists& nl, const ModelView& m, const SeqView& q, const TableView& in,
                            const TableView& out, int d, int i, int kind, int node) {
  const bool cE = d >= 2, cP = d >= 2 && q.pair_ok(i + 1, d - 2);
  double a = 0.;
  for (int e = nl.begin(kind, node); e < nl.end(kind, node); ++e) {
    const int32_t* t = nl.ent(e);
    const int s = t[0], sp = t[1];
    const double o = f.ld(out, ST_P, d, i, s);
    if (f.dead(o)) continue;
    const double ow = f.mul(o, f.w_pair2(m, q, s, sp, t[2], i, i + d - 1));
    if (cE) a += f.post(f.mul(ow, f.ld(in, ST_E, d - 2, i + 1, sp)));                                                   // 1a
    if (cP) a += f.post(f.mul(ow, f.mul(f.ld(in, ST_P, d - 2, i + 1, sp), f.w_stack(m, q, s, q.cell(i, d)))));          // 1b
  }
  return a;
}

// the cell [i, i + d), d >= 1, i + d <= L: the posterior that its right base j-1 is emitted by `node` in a rule applied at this
// cell (L <- L, 3a, the right base of 1a / 1b).  Lists in their order, L first.
template <class F>
ELEMDP_HD double node_cell_right(const F& f, const NodeLists& nl, const ModelView& m, const SeqView& q, const TableView& in,
                                 const TableView& out, int d, int i, int node) {
  const int j = i + d;
  double a = 0.;
  if (nl.rules & NR_LOOP)
  for (int e = nl.begin(NK_L, node); e < nl.end(NK_L, node); ++e) {
    const int s = nl.ent(e)[0];
    const double inL = f.ld(in, ST_L, d, i, s);
    if (f.dead(inL)) continue;
    a += f.post(f.mul(inL, f.ld(out, ST_L, d, i, s)));
  }
  if ((nl.rules & NR_3A) && q.unp[j - 1]) {
    if (q.left_ok(i, d) && q.left_ok(i, d - 1))
      for (int e = nl.begin(NK_R, node); e < nl.end(NK_R, node); ++e) {
        const int32_t* t = nl.ent(e);
        const double o = f.ld(out, ST_2, d, i, t[0]);
        if (f.dead(o)) continue;
        a += f.post(f.mul(o, f.mul(f.ld(in, ST_2, d - 1, i, t[1]), f.w_emit(m, q, t[0], t[2], j - 1))));
      }
    const int dmi = q.dmin[i];
    if (dmi > 0 && dmi < d - 1) a += f.chain(nl, m, q, in, out, d, i, node);
  }
  if ((nl.rules & NR_PAIR_R) && q.pair_ok(i, d)) a += node_pairs(f, nl, m, q, in, out, d, i, NK_PR, node);
  return a;
}

// the cell [i, i + d), d >= 1, i + d <= L: the posterior that its left base i is emitted by `node` (5a, the left base of 1a / 1b)
template <class F>
ELEMDP_HD double node_cell_left(const F& f, const NodeLists& nl, const ModelView& m, const SeqView& q, const TableView& in,
                                const TableView& out, int d, int i, int node) {
  double a = 0.;
  if ((nl.rules & NR_5A) && m_ok(m, q, i, d) && m_ok(m, q, i + 1, d - 1) && q.unp[i])
    for (int e = nl.begin(NK_M, node); e < nl.end(NK_M, node); ++e) {
      const int32_t* t = nl.ent(e);
      const double o = f.ld(out, ST_M, d, i, t[0]);
      if (f.dead(o)) continue;
      a += f.post(f.mul(o, f.mul(f.ld(in, ST_M, d - 1, i + 1, t[1]), f.w_left(m, q, t[1], t[2], i))));
    }
  if ((nl.rules & NR_PAIR_L) && q.pair_ok(i, d)) a += node_pairs(f, nl, m, q, in, out, d, i, NK_PL, node);
  return a;
}

// rule 8 at position p by `node`
template <class F>
ELEMDP_HD double node_exterior(const F& f, const NodeLists& nl, const ModelView& m, const SeqView& q, const TableView& in,
                               const TableView& out, int p, int node) {
  double a = 0.;
  if (!(nl.rules & NR_EXT) || !q.unp[p]) return a;
  for (int e = nl.begin(NK_R, node); e < nl.end(NK_R, node); ++e) {
    const int32_t* t = nl.ent(e);
    const double o = out.o(p + 1, t[0]);
    if (f.dead(o)) continue;
    a += f.post(f.mul(o, f.mul(in.o(p, t[1]), f.w_emit(m, q, t[0], t[2], p))));
  }
  return a;
}

// the cells of position p dealt to `part` of `nparts` by d (d = 1 + part, 1 + part + nparts, ..): per d the cell whose right base
// is p, then the cell whose left base is p
template <class F>
ELEMDP_HD double node_cells_part(const F& f, const NodeLists& nl, const ModelView& m, const SeqView& q, const TableView& in,
                                 const TableView& out, int p, int node, int part, int nparts) {
  double a = 0.;
  for (int d = 1 + part; d <= q.W; d += nparts) {
    if (d <= p + 1) a += node_cell_right(f, nl, m, q, in, out, d, p + 1 - d, node);
    if (p + d <= q.L) a += node_cell_left(f, nl, m, q, in, out, d, p, node);
  }
  return a;
}

ELEMDP_HD double node_finish(double cells, double ext) { return ctx_clamp(cells + ext); }
ELEMDP_HD double node_no_parse(int node) { return node == 0 ? 1. : 0.; }

// N(p, node), serial (the CPU driver, the log-space form); cells false: a model without secondary structure
template <class F>
ELEMDP_HD double node_value(const F& f, const NodeLists& nl, const ModelView& m, const SeqView& q, const TableView& in,
                            const TableView& out, int p, int node, bool cells) {
  return node_finish(cells ? node_cells_part(f, nl, m, q, in, out, p, node, 0, 1) : 0., node_exterior(f, nl, m, q, in, out, p, node));
}

}  // namespace elemdp
