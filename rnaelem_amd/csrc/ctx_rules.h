// ctx_rules.h -- structural context profiles under the motif model, host / device.
//
// For every position p of a sequence the probability that it is exterior (O), the left (L) or right (R) base of a pair, or
// unpaired in a hairpin (H), bulge (B), interior (I) or multi-branch (M) loop: the marginals of the rss letters of a parse,
// over the ensemble of the scan's first sum pass (terminals ari and nasi -- the ensemble of pair_rules.h), from its inside and
// outside tables.  Cell [i, j), d = j - i, Z = Z(ari, nasi); every table product below is divided by Z:
//
//   P(i, d)  pair posterior of pair_rules.h                                       L(p) = sum_d P(p, d),  R(p) = sum_i P(i, p+1-i)
//   u(i, d)  = sum_s in(L, i, j, s) out(L, i, j, s)                               U(p) = sum_i u(i, p+1-i)
//            every L entry with j > i is made by one L <- L emission at j-1, so U(p) is "p is unpaired in a run below a pair"
//   h(i, d)  = sum_s out(E, i, j, s) exp(lam(s) hairpin_energy(i-1, j)) in(L, i, j, s)      (rule 6b: the run [i, j) is a hairpin)
//   b(i, d)  = sum over the rule-6c items of the inside pass in which [i, j) is the only non-empty run:
//              as the left run  (outer E(i, l), inner P(j, l), empty right run L(l, l)) and
//              as the right run (outer E(k, j), inner P(k, i), empty left run L(k, k)), each
//              out(E, outer, par) exp(lam(par) loop_energy) in(P, inner, s1) in(L, empty, .) in(L, i, j, s)
//   h and b are posteriors of the whole run: each adds to every position of [i, j) -- a range-add, done as a difference array
//   over positions (+ at i, - at j) and a prefix sum in increasing position:   H(p), B(p)
//   I(p)     = max(0, U - H - B)                                                  (the runs of the other rule-6c items)
//   O(p)     = sum_s sum_{s1 in right(s)} out_o(p+1, s) wt in_o(p, s1)            (rule 8 at p)
//   M(p)     = max(0, 1 - L - R - U - O)
//
// The two remainders make a row sum to 1; they are exact wherever the tables' inside and outside agree.  With max_iloop < 30
// the outside pass enumerates interior loops the inside pass does not (SURVEY §7 quirk ii): the tables carry that, the pair
// posteriors inherit it and so do U, I and M here; hence the clamps at 0.  A sequence without a parse has O = 1 and 0 elsewhere,
// and so has every sequence of a model without secondary structure (ELEMDP_NO_RSS).
//
// One rule for both forms, as PairLin / PairLog: the compact scaled-linear tables (CtxLin; ctx_kernels.hip) and the dense
// log-space tables of the fused scan kernel (CtxLog).  Liveness is decided before every load, by control flow, never by a
// multiply: plane L is stored at every cell, plane E is read under e_ok alone, and the cells of an item (its outer E, its inner
// P) exist by the plan; the compact tables hold garbage where nothing is stored.  A scan keeps no per-item weight array
// (LinArgs::xwi is null: the band kernels form the weights where they stage the records), so the weight of an item is formed
// here from its energy.
//
// Rounding: in the scaled-linear form a row sums to 1 within a few ulp (1e-12 is what the tests hold).  In the log-space form a
// term is exp(a + b - ln Z), whose exponent carries eps |ln Z| of rounding, so rows sum to 1 within about 1e-15 |ln Z| per term
// (1e-10 is what the tests hold for sequences that left the double range).
#pragma once
#include "lin_rules.h"
#include "pair_rules.h"

namespace elemdp {

enum CtxCol : int { CTX_O = 0, CTX_L = 1, CTX_R = 2, CTX_H = 3, CTX_B = 4, CTX_I = 5, CTX_M = 6, CTX_COLS = 7 };

struct CtxLin {
  double invZ;   // 1 / the mantissa of Z(ari, nasi) in the tables' scale: every product below spans the whole sequence, as Z does
  ELEMDP_HD double ld(const TableView& T, int e, int d, int i, int s) const { return T.ld(e, d, i, s); }
  ELEMDP_HD bool dead(double v) const { return v == 0.; }
  ELEMDP_HD double mul(double a, double b) const { return a * b; }
  ELEMDP_HD double w_hairpin(const ModelView& m, const SeqView& q, int s, int c_up) const { return xw_cell(q, lamk(m, s), XT_HP, c_up); }
  // weight of a rule-6c item for lambda class k, from its energy (the engine keeps no per-item weights: the band kernels form them
  // where they stage the records, and so does this rule)
  ELEMDP_HD double w_item(const ModelView& m, int k, double tsc) const { return lin_weight(k ? m.lambda[1] : m.lambda[0], tsc); }
  ELEMDP_HD double w_emit(const ModelView& m, const SeqView& q, int par, int tf, int pos) const { return lw_right(m, q, par, tf, pos); }
  ELEMDP_HD double post(double v) const { return v * invZ; }
};
struct CtxLog {
  double lnZ;
  ELEMDP_HD double ld(const TableView& T, int e, int d, int i, int s) const { return T.at(e, d, i, s); }
  ELEMDP_HD bool dead(double v) const { return v == ELEMDP_NEG_INF; }
  ELEMDP_HD double mul(double a, double b) const { return a + b; }
  ELEMDP_HD double w_hairpin(const ModelView& m, const SeqView& q, int s, int c_up) const {
    const double e = q.e_hp[c_up];
    return e == ELEMDP_NEG_INF ? ELEMDP_NEG_INF : m.lam(s) * e;
  }
  ELEMDP_HD double w_item(const ModelView& m, int k, double tsc) const {
    return tsc == ELEMDP_NEG_INF ? ELEMDP_NEG_INF : (k ? m.lambda[1] : m.lambda[0]) * tsc;
  }
  ELEMDP_HD double w_emit(const ModelView& m, const SeqView& q, int par, int tf, int pos) const { return w_right(m, q, par, tf, pos); }
  ELEMDP_HD double post(double v) const { return v == ELEMDP_NEG_INF ? 0. : exp(v - lnZ); }
};

// the run [i, i + d), d >= 1, i + d <= L: u, h and b of the header.  u and h: states in increasing order.  b: the items of the
// run's by-left list, then of its by-right list, in list order -- the filter (one empty side, member of the inside enumeration)
// does not depend on the state, so a list is walked once --, and per item the loop states in increasing order and their tuples.
struct CtxCell { double u, h, b; };
template <class F>
ELEMDP_HD CtxCell ctx_cell(const F& f, const ModelView& m, const SeqView& q, const TableView& in, const TableView& out, int d, int i) {
  const AutomatonLayout& A = m.lay;
  const int32_t* I = m.ints;
  const int32_t* G = m.big;
  CtxCell c{0., 0., 0.};
  const bool eok = q.e_ok(i, d);
  const int c_up = eok ? q.cell(i - 1, d + 2) : 0;
  for (int s = 0; s < A.S; ++s) {
    if (!I[A.st_is_loop + s]) continue;
    const double inL = f.ld(in, ST_L, d, i, s);
    if (f.dead(inL)) continue;
    c.u += f.post(f.mul(inL, f.ld(out, ST_L, d, i, s)));
    if (eok) c.h += f.post(f.mul(inL, f.mul(f.ld(out, ST_E, d, i, s), f.w_hairpin(m, q, s, c_up))));
  }
  const int lc = q.cell(i, d);
  for (int n = q.by_left_off[lc]; n < q.by_left_off[lc + 1]; ++n) {          // left run of a bulge: the right run L(l, j) is empty
    const int idx = q.by_left_idx[n];
    const LoopItem it = q.items[idx];
    if (it.l != it.j || !q.item_in[idx]) continue;
    const double w0 = f.w_item(m, 0, it.tsc), w1 = f.w_item(m, 1, it.tsc);
    for (int s = 0; s < A.S; ++s) {
      if (!I[A.st_is_loop + s]) continue;
      const double inL = f.ld(in, ST_L, d, i, s);
      if (f.dead(inL)) continue;
      for (int u = G[A.quad2_off + s]; u < G[A.quad2_off + s + 1]; ++u) {
        const int par = G[A.quad2_ent + 3 * u], s1 = G[A.quad2_ent + 3 * u + 1], s3 = G[A.quad2_ent + 3 * u + 2];
        const double t = f.mul(f.ld(out, ST_E, it.j - it.i, it.i, par),
                               f.mul(f.ld(in, ST_P, it.l - it.k, it.k, s1), f.mul(f.ld(in, ST_L, 0, it.j, s3), lamk(m, par) ? w1 : w0)));
        c.b += f.post(f.mul(inL, t));
      }
    }
  }
  for (int n = q.by_right_off[lc]; n < q.by_right_off[lc + 1]; ++n) {        // right run of a bulge: the left run L(i, k) is empty
    const int idx = q.by_right_idx[n];
    const LoopItem it = q.items[idx];
    if (it.k != it.i || !q.item_in[idx]) continue;
    const double w0 = f.w_item(m, 0, it.tsc), w1 = f.w_item(m, 1, it.tsc);
    for (int s = 0; s < A.S; ++s) {
      if (!I[A.st_is_loop + s]) continue;
      const double inL = f.ld(in, ST_L, d, i, s);
      if (f.dead(inL)) continue;
      for (int u = G[A.quad3_off + s]; u < G[A.quad3_off + s + 1]; ++u) {
        const int par = G[A.quad3_ent + 3 * u], s1 = G[A.quad3_ent + 3 * u + 1], s2 = G[A.quad3_ent + 3 * u + 2];
        const double t = f.mul(f.ld(out, ST_E, it.j - it.i, it.i, par),
                               f.mul(f.ld(in, ST_P, it.l - it.k, it.k, s1), f.mul(f.ld(in, ST_L, 0, it.i, s2), lamk(m, par) ? w1 : w0)));
        c.b += f.post(f.mul(inL, t));
      }
    }
  }
  return c;
}

// O(p): rule 8 at position p, parents in increasing state order
template <class F>
ELEMDP_HD double ctx_exterior(const F& f, const ModelView& m, const SeqView& q, const TableView& in, const TableView& out, int p) {
  const AutomatonLayout& A = m.lay;
  const int32_t* I = m.ints;
  double a = 0.;
  if (!q.unp[p]) return a;
  for (int s = 0; s < A.S; ++s) {
    const double o = out.o(p + 1, s);
    if (f.dead(o)) continue;
    for (int t = I[A.right_off + s]; t < I[A.right_off + s + 1]; ++t)
      a += f.post(f.mul(o, f.mul(in.o(p, I[A.right_ent + 2 * t]), f.w_emit(m, q, s, I[A.right_ent + 2 * t + 1], p))));
  }
  return a;
}

// ---- from the per-run values to the profile.  X: one sequence's [i][d] array (rows of W+1, as P of pair_rules.h) with 0 where
// there is no run or pair.
// the runs that start at q, in increasing d
ELEMDP_HD double ctx_sum_from(const double* X, int L, int W, int q) {
  double a = 0.;
  for (int d = 1; d <= W && q + d <= L; ++d) a += X[(size_t)q * (W + 1) + d];
  return a;
}
// the runs that end in front of e (j = e), in increasing i
ELEMDP_HD double ctx_sum_to(const double* X, int L, int W, int e) {
  double a = 0.;
  for (int i = e - W < 0 ? 0 : e - W; i < e; ++i) a += X[(size_t)i * (W + 1) + (e - i)];
  return a;
}
// entry q of the difference array of a range-add of X(i, d) over [i, i + d): the prefix sum over 0 .. p is the sum of the
// runs that cover p
ELEMDP_HD double ctx_diff(const double* X, int L, int W, int q) { return ctx_sum_from(X, L, W, q) - ctx_sum_to(X, L, W, q); }

ELEMDP_HD double ctx_clamp(double v) { return v < 0. ? 0. : v > 1. ? 1. : v; }
// one row O L R H B I M from the sums of position p (h, b: the prefix sums of the difference arrays, which may round below 0)
ELEMDP_HD void ctx_compose(double o, double l, double r, double u, double h, double b, double* row) {
  h = ctx_clamp(h);
  b = ctx_clamp(b);
  row[CTX_O] = ctx_clamp(o); row[CTX_L] = ctx_clamp(l); row[CTX_R] = ctx_clamp(r);
  row[CTX_H] = h; row[CTX_B] = b;
  row[CTX_I] = ctx_clamp(u - h - b);
  row[CTX_M] = ctx_clamp(1. - l - r - u - o);
}
ELEMDP_HD void ctx_row_exterior(double* row) {   // no parse, or no secondary structure in the model
  row[CTX_O] = 1.;
  for (int c = 1; c < CTX_COLS; ++c) row[c] = 0.;
}

// the whole finish of one sequence, serial (the order of the CPU driver; ctx_kernels.hip forms the same prefix sums per tile)
ELEMDP_HD void ctx_finish(const double* P, const double* U, const double* H, const double* B, const double* O, int L, int W, double* profile) {
  double h = 0., b = 0.;
  for (int p = 0; p < L; ++p) {
    h += ctx_diff(H, L, W, p);
    b += ctx_diff(B, L, W, p);
    ctx_compose(O[p], ctx_sum_from(P, L, W, p), ctx_sum_to(P, L, W, p + 1), ctx_sum_to(U, L, W, p + 1), h, b, profile + (size_t)CTX_COLS * p);
  }
}

}  // namespace elemdp
