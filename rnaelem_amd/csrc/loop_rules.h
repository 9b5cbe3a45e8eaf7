// loop_rules.h -- loop posteriors under the motif model, host / device.
//
// For a kept cell [i, j), d = j - i >= 2 -- the pair of the bases i and j-1 -- the probability of what the pair closes, over the
// ensemble of the scan's first sum pass (terminals ari and nasi, Z = Z(ari, nasi): the ensemble of pair_rules.h, stem_rules.h and
// helix_rules.h), from its inside and outside tables.  in(P, i, d, .) is made by rule 1b -- the pair stacks on (i+1, j-1) -- or by
// rule 1a through the entry E(i', d'), (i', d') = (i+1, d-2), j' = i' + d', which is made by exactly one of rules 6a, 6b and 6c
// (sample_rules.h: TT_E_M, TT_E_H, TT_E_P).  With c = cell(i, d), every term divided by Z:
//
//   S(i, d) = sum_s out(P, i, d, s) sum_{(sp, tf) in pair(s)} wp(s, sp, tf, i, j-1) in(P, i+1, d-2, sp) xst(s, c)
//             under pair_ok(i+1, d-2): the 1b term of stem_rules.h over all slots, H(i, d, 2) of helix_rules.h
//   H(i, d) = sum_{s loop state} out(E, i', d', s) w_hairpin(s, c) in(L, i', d', s)              rule 6b, h(i', d') of ctx_rules.h
//   M(i, d) = sum_s out(E, i', d', s) w_close(s, c) in(M, i', d', s)                              rule 6a, under m_ok(i', d')
//   T(item) = sum_s out(E, i', d', s) w_item(lamk(s), tsc)
//                   sum_{(s1, s2, s3) in quad(s)} in(P, k, l-k, s1) in(L, i', k-i', s2) in(L, l, j'-l, s3)       rule 6c
//             for the items of the outer cell (i', d') in by_outer order that belong to the inside enumeration (item_in) and whose
//             inner cell [k, l) is kept: the two-loop "(i, j) directly around (k, l)"
//   B(i, d) = sum of T over the items with one empty run (k = i' or l = j'),  I(i, d) = sum of T over the others
//
// M is the probability of the closing event alone, whatever the shape of the multi-branch loop: the joint probability of one
// particular multi-loop with all its branches is a path through rules 2 to 5 and is not formed here.  Every value is clamped to
// [0, 1]; nothing is renormalised.  H + S + B + I + M is the P of pair_rules.h and T <= P wherever the tables' inside and outside
// agree; with max_iloop < 30 the outside pass enumerates interior loops the inside pass does not (SURVEY §7 quirk ii), the outside
// tables carry that and the five columns may fall short of P.
//
// One rule for both forms (LoopLin: the compact scaled-linear tables; LoopLog: the dense log-space tables of the fused scan kernel);
// the weights are those of the existing policies (w_pair2, w_stack, w_hairpin, w_item) and the XT_CLOSE weight of sample_rules.h.
// Liveness is decided before every load, by control flow, never by a multiply; the caller holds pair_ok(i, d) and d >= 2, and a cell
// that is not kept is never read.  Every function is the work of one lane (OneLane of access_rules.h): the states in increasing
// order, the lists in list order, so a value is a function of the tables' bits.  loop_two takes out(E, i', d', .) through a functor:
// the table itself (the CPU driver, the log-space form, the loops of a caller-given structure), or the copy a wave of
// loop_kernels.hip staged in LDS for all the items of one outer cell -- the same values, hence the same bits.
#pragma once
#include "helix_rules.h"

namespace elemdp {

enum LoopType : int { LOOP_NONE = 0, LOOP_H = 1, LOOP_S = 2, LOOP_B = 3, LOOP_I = 4, LOOP_M = 5 };
// the columns of the closing list, in the order of the types
enum LoopCol : int { LC_H = 0, LC_S = 1, LC_B = 2, LC_I = 3, LC_M = 4, LOOP_COLS = 5 };

struct LoopLin : HelixLin {
  ELEMDP_HD explicit LoopLin(double invZ_) : HelixLin(invZ_) {}
  ELEMDP_HD double w_close(const ModelView& m, const SeqView& q, int s, int c) const { return xw_cell(q, lamk(m, s), XT_CLOSE, c); }
};
struct LoopLog : HelixLog {
  ELEMDP_HD explicit LoopLog(double lnZ_) : HelixLog(lnZ_) {}
  ELEMDP_HD double w_close(const ModelView& m, const SeqView& q, int s, int c) const {
    const double e = q.e_close[c];
    return e == ELEMDP_NEG_INF ? ELEMDP_NEG_INF : m.lam(s) * e;
  }
};

// S: the pair (i, j-1) stacks on (i+1, j-2)
template <class F>
ELEMDP_HD double loop_stack(const F& f, const ModelView& m, const SeqView& q, const TableView& in, const TableView& out, int i, int d) {
  const AutomatonLayout& A = m.lay;
  const int32_t* I = m.ints;
  if (d - 2 < 2 || !q.pair_ok(i + 1, d - 2)) return 0.;
  const int c = q.cell(i, d);
  double a = 0.;
  for (int s = 0; s < A.S; ++s) {
    if (I[A.pair_off + s] == I[A.pair_off + s + 1]) continue;
    const double o = f.ld(out, ST_P, d, i, s);
    if (f.dead(o)) continue;
    const double xs = f.w_stack(m, q, s, c);
    if (f.dead(xs)) continue;
    for (int t = I[A.pair_off + s]; t < I[A.pair_off + s + 1]; ++t) {
      const int sp = I[A.pair_ent + 2 * t], tf = I[A.pair_ent + 2 * t + 1];
      const double ow = f.mul(o, f.w_pair2(m, q, s, sp, tf, i, i + d - 1));
      a += f.post(f.mul(ow, f.mul(f.ld(in, ST_P, d - 2, i + 1, sp), xs)));
    }
  }
  return ctx_clamp(a);
}

// H: the pair closes a hairpin (the product of ctx_cell's h, term by term)
template <class F>
ELEMDP_HD double loop_hairpin(const F& f, const ModelView& m, const SeqView& q, const TableView& in, const TableView& out, int i, int d) {
  const AutomatonLayout& A = m.lay;
  const int32_t* I = m.ints;
  const int ie = i + 1, de = d - 2, c = q.cell(i, d);
  double a = 0.;
  for (int s = 0; s < A.S; ++s) {
    if (!I[A.st_is_loop + s]) continue;
    const double w = f.w_hairpin(m, q, s, c);
    if (f.dead(w)) continue;
    const double inL = f.ld(in, ST_L, de, ie, s);
    if (f.dead(inL)) continue;
    a += f.post(f.mul(inL, f.mul(f.ld(out, ST_E, de, ie, s), w)));
  }
  return ctx_clamp(a);
}

// M: the pair closes a multi-branch loop, of any shape
template <class F>
ELEMDP_HD double loop_multi(const F& f, const ModelView& m, const SeqView& q, const TableView& in, const TableView& out, int i, int d) {
  const AutomatonLayout& A = m.lay;
  const int ie = i + 1, de = d - 2, c = q.cell(i, d);
  if (!m_ok(m, q, ie, de)) return 0.;
  double a = 0.;
  for (int s = 0; s < A.S; ++s) {
    const double w = f.w_close(m, q, s, c);   // (dead where e_close[c] is not finite)
    if (f.dead(w)) continue;
    const double o = f.ld(out, ST_E, de, ie, s);
    if (f.dead(o)) continue;
    a += f.post(f.mul(o, f.mul(f.ld(in, ST_M, de, ie, s), w)));
  }
  return ctx_clamp(a);
}

// T of the item x of the outer cell (ie, de) = (i+1, d-2); the caller checked item_in and pair_ok of the inner cell.  oe(s) is
// out(E, ie, de, s).
template <class F, class OE>
ELEMDP_HD double loop_two(const F& f, const ModelView& m, const SeqView& q, const TableView& in, OE oe, int ie, int de, const LoopItem& x) {
  const AutomatonLayout& A = m.lay;
  const int32_t* G = m.big;
  const int je = ie + de;
  const double w0 = f.w_item(m, 0, x.tsc), w1 = f.w_item(m, 1, x.tsc);
  double a = 0.;
  for (int s = 0; s < A.S; ++s) {
    const int t0 = G[A.quad_off + s], t1 = G[A.quad_off + s + 1];
    if (t0 == t1) continue;
    const double w = lamk(m, s) ? w1 : w0;
    if (f.dead(w)) continue;
    const double o = oe(s);
    if (f.dead(o)) continue;
    double inner = f.zero();
    for (int t = t0; t < t1; ++t) {
      const double p = f.ld(in, ST_P, x.l - x.k, x.k, G[A.quad_ent + 3 * t]);
      if (f.dead(p)) continue;
      const double l2 = f.ld(in, ST_L, x.k - ie, ie, G[A.quad_ent + 3 * t + 1]);
      if (f.dead(l2)) continue;
      const double l3 = f.ld(in, ST_L, je - x.l, x.l, G[A.quad_ent + 3 * t + 2]);
      if (f.dead(l3)) continue;
      inner = f.add(inner, f.mul(p, f.mul(l2, l3)));
    }
    if (f.dead(inner)) continue;
    a += f.post(f.mul(f.mul(o, w), inner));
  }
  return ctx_clamp(a);
}

// an item of the outer cell (ie, de) counts where it belongs to the inside enumeration and its inner cell is kept
ELEMDP_HD bool loop_item_live(const SeqView& q, int it) {
  if (!q.item_in[it]) return false;
  const LoopItem x = q.items[it];
  return q.pair_ok(x.k, x.l - x.k);
}
ELEMDP_HD bool loop_item_bulge(const LoopItem& x) { return x.k == x.i || x.l == x.j; }

// the five columns of the kept cell [i, i + d), d >= 2, by one lane; T (null: not stored) receives the two-loop values at the
// items' by-outer positions (written for the live items alone)
template <class F>
ELEMDP_HD void loop_cell(const F& f, const ModelView& m, const SeqView& q, const TableView& in, const TableView& out, int i, int d,
                         double* cols, double* T) {
  const int ie = i + 1, de = d - 2;
  cols[LC_H] = loop_hairpin(f, m, q, in, out, i, d);
  cols[LC_S] = loop_stack(f, m, q, in, out, i, d);
  cols[LC_M] = loop_multi(f, m, q, in, out, i, d);
  double b = 0., n = 0.;
  const int oc = q.cell(ie, de);
  for (int it = q.by_outer_off[oc]; it < q.by_outer_off[oc + 1]; ++it) {
    if (!loop_item_live(q, it)) continue;
    const LoopItem x = q.items[it];
    const double t = loop_two(f, m, q, in, [&](int s) { return f.ld(out, ST_E, de, ie, s); }, ie, de, x);
    if (T) T[it] = t;
    if (loop_item_bulge(x)) b += t; else n += t;
  }
  cols[LC_B] = ctx_clamp(b);
  cols[LC_I] = ctx_clamp(n);
}

// one loop of a caller-given structure: the closing cell [i, i + d), its type, and for a bulge or an interior loop the inner cell
// [k, l).  0 exactly where the closing pair is no kept cell (a span above the band among them), where the inner pair of a stack is
// not kept, and where the two-loop is no item of the inside enumeration with a kept inner cell.
template <class F>
ELEMDP_HD double loop_of_structure(const F& f, const ModelView& m, const SeqView& q, const TableView& in, const TableView& out, int type,
                                   int i, int d, int k, int l) {
  if (d < 2 || !q.pair_ok(i, d)) return 0.;
  if (type == LOOP_H) return loop_hairpin(f, m, q, in, out, i, d);
  if (type == LOOP_S) return loop_stack(f, m, q, in, out, i, d);
  if (type == LOOP_M) return loop_multi(f, m, q, in, out, i, d);
  if (type != LOOP_B && type != LOOP_I) return 0.;
  const int ie = i + 1, de = d - 2, oc = q.cell(ie, de);
  for (int it = q.by_outer_off[oc]; it < q.by_outer_off[oc + 1]; ++it) {
    const LoopItem x = q.items[it];
    if (x.k != k || x.l != l) continue;
    if (!loop_item_live(q, it)) return 0.;
    return loop_two(f, m, q, in, [&](int s) { return f.ld(out, ST_E, de, ie, s); }, ie, de, x);
  }
  return 0.;
}

// An outer cell is walked where its P reaches min_prob less a margin of rounding (the margin of helix_kernels.hip's pick): T <= P
// up to rounding, so no entry of the two-loop list is lost, and the closing list itself is cut at min_prob exactly.
#if defined(__HIPCC__)
__host__
#endif
ELEMDP_HD double loop_pick_bound(double min_prob) { return min_prob * (1. - 1. / 1073741824.); }   // (2^-30)

// units of a slot's scratch (host): one per cell of the largest sequence, as helix_units_cap
inline size_t loop_units_cap(int Lmax, int Wmax) { return helix_units_cap(Lmax, Wmax); }

}  // namespace elemdp
