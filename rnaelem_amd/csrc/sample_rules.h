// sample_rules.h -- stochastic samples of whole derivations of the joint motif x energy grammar, host / device.
//
// The walk is trace_back (scan_rules.h) with sums in place of maxima and a random draw in place of the arg-max: every visited
// target (plane e, span d, start i, state s), or exterior target O(j, s), enumerates the candidates of its inside sum rule
// (lin_rules.h) from the finished inside table, and one candidate is drawn with probability w_k / tot.  A derivation is drawn
// with its exact probability under the model, and the sample reports the log of that probability.
//
// Candidate order (fixed; the lists of the inside sum rule, lin_inside_target_u / lin_inside_ext_part):
//   L  rule of the loop region: the right list (L(i, j-1, s1) x w_right)
//   P  per pair entry (the inside rule's order): rule 1a, then rule 1b
//   B  rule 2 by split point k ascending, then by state tuple: 1(i, k, s1) x 2(k, j, s2) -- read from planes 1 and 2, not from
//      the factorised pair tables; where a candidate of 1 or M is B itself, its weight is that sum (sample_bif), not plane B
//   2  rule 3a (right list), then 3b (P(i, j, s) x ml)
//   1  rule 4a (2), then 4b (B)
//   M  rule 5a (left list), then 5b (B)
//   E  rule 6a (M x close), 6b (L x hairpin), then 6c by item (by_outer order), then by state tuple
//   O  rule 7 by pair (i, j) with i descending, then by state tuple; then rule 8 (right list)
// Each weight is a product of its children's table values and its transition weight, rounded (ELEMDP_MUL_RN) as the sum pass
// rounds its products (in the log form: a sum of logs).  tot = sum of w_k in that order; the draw u in [0, 1) picks the first k with u * tot < w_0 + .. + w_k,
// or, if rounding leaves none, the last k with w_k > 0.
//
// Every candidate of one target covers the same positions, so the ratios w_k / tot are free of the per-position scale of the
// scaled-linear tables.  The walk reads tables through a form (LinSampleTab: the compact tables of the
// scaled-linear sweeps; LogSampleTab: the dense log tables of the fused scan kernel), and only live entries, with the liveness
// discipline of lin_rules.h.
#pragma once
#include <cmath>
#include <cstdint>

#include "lin_rules.h"
#include "scan_rules.h"

namespace elemdp {

// ---- the generator: a pure function of (seed, sequence index, sample index, draw index) -------------------------------------
//   mix(x)  = SplitMix64's output function of x + 0x9E3779B97F4A7C15:
//             z = x + 0x9E3779B97F4A7C15;  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;  z = (z ^ (z >> 27)) * 0x94D049BB133111EB;
//             return z ^ (z >> 31)                                            (all arithmetic mod 2^64)
//   key     = mix(mix(mix(mix(seed) ^ index) ^ sample) ^ draw)
//   u       = (key >> 11) * 2^-53                                             (53 bits, in [0, 1))
// index = batch index + index_base (elemdp_sample); draw 0 picks the terminal state, draw t >= 1 the t-th visited target.
ELEMDP_HD uint64_t sample_mix(uint64_t x) {
  uint64_t z = x + 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
ELEMDP_HD double sample_uniform(uint64_t seed, uint64_t index, uint64_t sample, uint64_t draw) {
  const uint64_t k = sample_mix(sample_mix(sample_mix(sample_mix(seed) ^ index) ^ sample) ^ draw);
  return (double)(k >> 11) * (1.0 / 9007199254740992.0);
}

// status per sequence (elemdp_sample)
enum SampleStatus : int32_t { SAMPLE_OK = 0, SAMPLE_NO_PARSE = 1, SAMPLE_REFUSED = 2 };

// Table access and arithmetic of the walk (the "form").  A form gives the children's table values (every load names its
// liveness), the product of values, the transition weights, the sum of the candidates (tot) and the weight of candidate v in
// tot.  Two forms:
//   LinSampleTab  the compact tables of the scaled-linear sweeps: values are scaled Boltzmann weights, products rounded
//                 (ELEMDP_MUL_RN), tot a plain sum, candidate k drawn where u * tot < w_0 + .. + w_k
//   LogSampleTab  the dense log tables of the fused scan kernel: values are logs, products are sums, tot = log-sum-exp (lse2) of
//                 the candidates in the same order, candidate k drawn where u < exp(v_0 - tot) + .. + exp(v_k - tot)
struct LinSampleTab {
  const TableView& T;
  ELEMDP_HD double ld(int e, int d, int i, int s, bool live) const { return T.ld(e, d, i, s, live); }
  ELEMDP_HD double o(int j, int s) const { return T.o(j, s); }
  ELEMDP_HD static double mul(double a, double b) { return ELEMDP_MUL_RN(a, b); }
  ELEMDP_HD static double zero() { return 0.; }
  ELEMDP_HD static double add(double acc, double v) { return acc + v; }
  ELEMDP_HD static bool pos(double v) { return v > 0.; }
  ELEMDP_HD static double thresh(double u, double tot) { return u * tot; }
  ELEMDP_HD static double w(double v, double) { return v; }
  ELEMDP_HD static double lp(double v, double tot) { return log(v) - log(tot); }
  ELEMDP_HD static double wr(const ModelView& m, const SeqView& q, int par, int tf, int pos) { return lw_right(m, q, par, tf, pos); }
  ELEMDP_HD static double wl(const ModelView& m, const SeqView& q, int ch, int tf, int pos) { return lw_left(m, q, ch, tf, pos); }
  ELEMDP_HD static double wp(const ModelView& m, const SeqView& q, int par, int ch, int tf, int pi, int pj) {
    return lw_pair(m, q, par, ch, tf, pi, pj);
  }
  // structural term `term` of cell c under the lambda class of state s (the exponentials of Engine::lin_weights)
  ELEMDP_HD static double xc(const ModelView& m, const SeqView& q, int s, int term, int c) { return xw_cell(q, lamk(m, s), term, c); }
  // interior-loop item: the band kernels of the scan form exp(lambda tsc) where they stage the items (no item table)
  ELEMDP_HD static double xi(const ModelView& m, int s, double tsc) { return lin_weight(m.lam(s), tsc); }
};
struct LogSampleTab {
  const TableView& T;
  ELEMDP_HD double ld(int e, int d, int i, int s, bool live) const { return live ? T.ldm(e, d, i, s) : ELEMDP_NEG_INF; }
  ELEMDP_HD double o(int j, int s) const { return T.o(j, s); }
  ELEMDP_HD static double mul(double a, double b) { return a + b; }
  ELEMDP_HD static double zero() { return ELEMDP_NEG_INF; }
  ELEMDP_HD static double add(double acc, double v) { return lse2(acc, v); }
  ELEMDP_HD static bool pos(double v) { return v > ELEMDP_NEG_INF && v < HUGE_VAL; }
  ELEMDP_HD static double thresh(double u, double) { return u; }
  ELEMDP_HD static double w(double v, double tot) { return exp(v - tot); }
  ELEMDP_HD static double lp(double v, double tot) { return v - tot; }
  ELEMDP_HD static double wr(const ModelView& m, const SeqView& q, int par, int tf, int pos) { return w_right(m, q, par, tf, pos); }
  ELEMDP_HD static double wl(const ModelView& m, const SeqView& q, int ch, int tf, int pos) { return w_left(m, q, ch, tf, pos); }
  ELEMDP_HD static double wp(const ModelView& m, const SeqView& q, int par, int ch, int tf, int pi, int pj) {
    return w_pair(m, q, par, ch, tf, pi, pj);
  }
  ELEMDP_HD static double xc(const ModelView& m, const SeqView& q, int s, int term, int c) {
    const double* t = term == XT_STACK ? q.e_stack : term == XT_EXT ? q.e_ext : term == XT_ML ? q.e_ml : term == XT_CLOSE ? q.e_close : q.e_hp;
    const double e = t[c];
    return e == ELEMDP_NEG_INF ? ELEMDP_NEG_INF : ELEMDP_MUL_RN(m.lam(s), e);
  }
  ELEMDP_HD static double xi(const ModelView& m, int s, double tsc) {
    return tsc == ELEMDP_NEG_INF ? ELEMDP_NEG_INF : ELEMDP_MUL_RN(m.lam(s), tsc);
  }
};

// one candidate: the transition (TT_*), the interval (k, l) of its first child, the child's plane, and up to three states
// (s1: the first child; s2: the second child of rules 2 and 7, the left loop of rule 6c; s3: the right loop of rule 6c)
struct SampleStep {
  int16_t k, l;
  int8_t t, e1;
  int16_t s1, s2, s3;
};

// rule 2 by split point k ascending, then by state tuple: f(1(i, k, s1) x 2(k, j, s2), k, s1, s2) for left_ok(i, d).  Plane B itself
// is not read: the table-driven unary phases (lin_fast.h) fold B into planes 1 and M without storing it.
template <class Tab, class F>
ELEMDP_HD void sample_split(const ModelView& m, const SeqView& q, const Tab& T, int d, int i, int s, F f) {
  const AutomatonLayout& A = m.lay;
  const int32_t* G = m.big;
  const int j = i + d;
  for (int k = i + q.dmin[i]; k < j; ++k) {
    const int dk = q.dmin[k];
    if (dk == 0 || j - k < dk) continue;
    for (int t = G[A.split_off + s]; t < G[A.split_off + s + 1]; ++t) {
      const int s1 = G[A.split_ent + 2 * t], s2 = G[A.split_ent + 2 * t + 1];
      f(T.mul(T.ld(ST_1, k - i, i, s1, true), T.ld(ST_2, j - k, k, s2, true)), k, s1, s2);
    }
  }
}
// B(i, d, s) as the sum of those candidates, in that order
template <class Tab>
ELEMDP_HD double sample_bif(const ModelView& m, const SeqView& q, const Tab& T, int d, int i, int s) {
  double b = T.zero();
  sample_split(m, q, T, d, i, s, [&](double w, int, int, int) { b = T.add(b, w); });
  return b;
}

// calls f(w, step) for every candidate of target (e, d, i, s) (e = ST_O: exterior target O(j = i, s)) in the order above
template <class Tab, class F>
ELEMDP_HD void sample_candidates(const ModelView& m, const SeqView& q, const Tab& T, int e, int d, int i, int s, F f) {
  const AutomatonLayout& A = m.lay;
  const int32_t* I = m.ints;
  const int32_t* G = m.big;
  auto step = [](int k, int l, int t, int e1, int s1, int s2 = -1, int s3 = -1) {
    SampleStep x;
    x.k = (int16_t)k; x.l = (int16_t)l; x.t = (int8_t)t; x.e1 = (int8_t)e1;
    x.s1 = (int16_t)s1; x.s2 = (int16_t)s2; x.s3 = (int16_t)s3;
    return x;
  };
  if (e == ST_O) {
    const int j = i;
    if (j == 0) return;
    const int i0 = (j - q.W > 0) ? j - q.W : 0;
    for (int a = j - 1; a >= i0; --a) {   // rule 7
      const int da = j - a;
      if (!q.pair_ok(a, da)) continue;
      const double xe = T.xc(m, q, s, XT_EXT, q.cell(a, da));
      for (int u = G[A.split_off + s]; u < G[A.split_off + s + 1]; ++u) {
        const int s2 = G[A.split_ent + 2 * u], s1 = G[A.split_ent + 2 * u + 1];
        f(T.mul(T.mul(T.o(a, s2), T.ld(ST_P, da, a, s1, true)), xe), step(a, j, TT_O_OP, ST_P, s1, s2));
      }
    }
    if (q.unp[j - 1])   // rule 8
      for (int t = I[A.right_off + s]; t < I[A.right_off + s + 1]; ++t) {
        const int s1 = I[A.right_ent + 2 * t], tf = I[A.right_ent + 2 * t + 1];
        f(T.mul(T.o(j - 1, s1), T.wr(m, q, s, tf, j - 1)), step(0, j - 1, TT_O_O, ST_O, s1));
      }
    return;
  }
  const int j = i + d;
  const bool isloop = I[A.st_is_loop + s] != 0;
  const bool pok = q.pair_ok(i, d), lok = q.left_ok(i, d), mok = m_ok(m, q, i, d), eok = q.e_ok(i, d);
  switch (e) {
    case ST_L:
      if (!isloop || d == 0) return;
      for (int t = I[A.right_off + s]; t < I[A.right_off + s + 1]; ++t) {
        const int s1 = I[A.right_ent + 2 * t], tf = I[A.right_ent + 2 * t + 1];
        f(T.mul(T.ld(ST_L, d - 1, i, s1, true), T.wr(m, q, s, tf, j - 1)), step(i, j - 1, TT_L_L, ST_L, s1));
      }
      return;
    case ST_P: {
      if (!pok || d < 2) return;
      const bool cP = q.pair_ok(i + 1, d - 2);
      const double xst = T.xc(m, q, s, XT_STACK, q.cell(i, d));
      for (int t = I[A.pair_off + s]; t < I[A.pair_off + s + 1]; ++t) {   // per pair entry: 1a, then 1b (lin_inside_target_u)
        const int s1 = I[A.pair_ent + 2 * t], tf = I[A.pair_ent + 2 * t + 1];
        const double wpr = T.wp(m, q, s, s1, tf, i, j - 1);
        f(T.mul(wpr, T.ld(ST_E, d - 2, i + 1, s1, true)), step(i + 1, j - 1, TT_P_E, ST_E, s1));
        if (cP) f(T.mul(wpr, T.mul(T.ld(ST_P, d - 2, i + 1, s1, true), xst)), step(i + 1, j - 1, TT_P_P, ST_P, s1));
      }
      return;
    }
    case ST_B:
      if (!lok) return;
      sample_split(m, q, T, d, i, s, [&](double w, int k, int s1, int s2) { f(w, step(i, k, TT_B_12, ST_1, s1, s2)); });
      return;
    case ST_2:
      if (!lok) return;
      if (q.left_ok(i, d - 1) && q.unp[j - 1])
        for (int t = I[A.right_off + s]; t < I[A.right_off + s + 1]; ++t) {
          const int s1 = I[A.right_ent + 2 * t], tf = I[A.right_ent + 2 * t + 1];
          f(T.mul(T.ld(ST_2, d - 1, i, s1, true), T.wr(m, q, s, tf, j - 1)), step(i, j - 1, TT_2_2, ST_2, s1));
        }
      if (pok) f(T.mul(T.ld(ST_P, d, i, s, true), T.xc(m, q, s, XT_ML, q.cell(i, d))), step(i, j, TT_2_P, ST_P, s));
      return;
    case ST_1:
      if (!lok) return;
      f(T.ld(ST_2, d, i, s, true), step(i, j, TT_1_2, ST_2, s));
      f(sample_bif(m, q, T, d, i, s), step(i, j, TT_1_B, ST_B, s));
      return;
    case ST_M:
      if (!mok) return;
      if (m_ok(m, q, i + 1, d - 1) && q.unp[i])
        for (int t = I[A.left_off + s]; t < I[A.left_off + s + 1]; ++t) {
          const int s1 = I[A.left_ent + 2 * t], tf = I[A.left_ent + 2 * t + 1];
          f(T.mul(T.ld(ST_M, d - 1, i + 1, s1, true), T.wl(m, q, s1, tf, i)), step(i + 1, j, TT_M_M, ST_M, s1));
        }
      if (lok) f(sample_bif(m, q, T, d, i, s), step(i, j, TT_M_B, ST_B, s));
      return;
    case ST_E: {
      if (!eok) return;
      const int c_up = q.cell(i - 1, d + 2);
      if (mok) f(T.mul(T.ld(ST_M, d, i, s, true), T.xc(m, q, s, XT_CLOSE, c_up)), step(i, j, TT_E_M, ST_M, s));
      if (isloop) f(T.mul(T.ld(ST_L, d, i, s, true), T.xc(m, q, s, XT_HP, c_up)), step(i, j, TT_E_H, ST_L, s));
      const int c0 = q.by_outer_off[q.cell(i, d)], c1 = q.by_outer_off[q.cell(i, d) + 1];
      for (int it = c0; it < c1; ++it) {
        if (!q.item_in[it]) continue;
        const LoopItem x = q.items[it];
        const bool live = q.pair_ok(x.k, x.l - x.k);
        const double xw = T.xi(m, s, x.tsc);
        for (int t = G[A.quad_off + s]; t < G[A.quad_off + s + 1]; ++t) {
          const int s1 = G[A.quad_ent + 3 * t], s2 = G[A.quad_ent + 3 * t + 1], s3 = G[A.quad_ent + 3 * t + 2];
          const double w = T.mul(
              T.mul(T.ld(ST_P, x.l - x.k, x.k, s1, live),
                            T.mul(T.ld(ST_L, x.k - i, i, s2, true), T.ld(ST_L, j - x.l, x.l, s3, true))),
              xw);
          f(w, step(x.k, x.l, TT_E_P, ST_P, s1, s2, s3));
        }
      }
      return;
    }
    default: return;
  }
}

// the drawn candidate of a target, or t = -1 when it has none with w > 0; adds log w_k - log tot to *logp
template <class Tab>
ELEMDP_HD SampleStep sample_target(const ModelView& m, const SeqView& q, const Tab& T, int e, int d, int i, int s, double u,
                                   double* logp) {
  double tot = T.zero();
  sample_candidates(m, q, T, e, d, i, s, [&](double v, const SampleStep&) { tot = T.add(tot, v); });
  SampleStep pick, last;
  pick.t = last.t = -1;
  double vp = 0., vl = 0.;
  if (T.pos(tot)) {
    const double x = T.thresh(u, tot);
    double pre = 0.;
    sample_candidates(m, q, T, e, d, i, s, [&](double v, const SampleStep& c) {
      if (pick.t >= 0) return;
      const double w = T.w(v, tot);
      pre += w;
      if (w > 0.) { last = c; vl = v; }
      if (x < pre && w > 0.) { pick = c; vp = v; }
    });
  }
  if (pick.t < 0) { pick = last; vp = vl; }
  if (pick.t >= 0) *logp += T.lp(vp, tot);
  return pick;
}

// frames that draw nothing and write nothing: the empty loop region L(i, i) and the start of the chain O(0)
ELEMDP_HD bool sample_leaf(int e, int i, int j) { return (e == ST_L && i == j) || (e == ST_O && j == 0); }

// Stack bound of sample_walk: the pending frames cover disjoint, non-empty intervals of [0, L) (leaves are never pushed), so at
// most L of them; + 4 for the frames one step pushes before the bound is checked.
constexpr int sample_stack_cap(int L) { return L + 4; }

// One sample: the terminal state among s00, s0m2, s0m1 by O(L, .) (draw 0), then the walk from O(L, s0) with frame handling and
// writes as in trace_back: the motif node per position (node), the structure letters O L R H B I M (rss), and the log of the
// derivation's probability (*logp).  Returns SAMPLE_OK, SAMPLE_NO_PARSE (Z = 0), or SAMPLE_REFUSED (no candidate with w > 0 at a
// visited target, or more than cap frames).  world (option world): 1 = the terminal is drawn among s0m2 and s0m1
// alone (the parses with the motif), 2 = it is s00 (the parses without it); Z, the draw and *logp are that world's, draw 0 is
// consumed either way, an empty world is SAMPLE_NO_PARSE.
template <class Tab>
ELEMDP_HD int sample_walk(const ModelView& m, const SeqView& q, const Tab& T, uint64_t seed, uint64_t index, uint64_t sample,
                          uint8_t* node, char* rss, double* logp, TraceFrame* stack, int cap, int world = 0) {
  const AutomatonLayout& A = m.lay;
  const int32_t* I = m.ints;
  const int L = q.L;
  *logp = 0.;
  const int term[3] = {A.s00, A.s0m2, A.s0m1};
  double v[3], Z = T.zero();
  for (int k = 0; k < 3; ++k) {
    v[k] = (world == 1 && k == 0) || (world == 2 && k != 0) ? T.zero() : T.o(L, term[k]);
    Z = T.add(Z, v[k]);
  }
  if (!T.pos(Z)) return SAMPLE_NO_PARSE;
  uint64_t draw = 0;
  int s0 = -1;
  {
    const double x = T.thresh(sample_uniform(seed, index, sample, draw++), Z);
    double pre = 0.;
    int last = -1;
    for (int k = 0; k < 3 && s0 < 0; ++k) {
      const double w = T.w(v[k], Z);
      pre += w;
      if (w > 0.) last = k;
      if (x < pre && w > 0.) s0 = k;
    }
    if (s0 < 0) s0 = last;
    *logp += T.lp(v[s0], Z);
    s0 = term[s0];
  }
  int top = 0;
  if (L > 0) stack[top++] = TraceFrame{0, (int16_t)L, (int8_t)ST_O, (int16_t)s0};
  auto push = [&](int i, int j, int e, int s) {
    if (!sample_leaf(e, i, j)) stack[top++] = TraceFrame{(int16_t)i, (int16_t)j, (int8_t)e, (int16_t)s};
  };
  while (top > 0) {
    const TraceFrame f = stack[--top];
    const int fi = (f.e == ST_O) ? f.j : f.i;   // (sample_candidates takes the exterior target's j in place of i)
    const SampleStep t = sample_target(m, q, T, f.e, f.j - f.i, fi, f.s, sample_uniform(seed, index, sample, draw++), logp);
    if (t.t < 0) return SAMPLE_REFUSED;
    if (top + 3 > cap) return SAMPLE_REFUSED;
    const int s1 = t.s1;
    const uint8_t fr = (uint8_t)I[A.st_r + f.s];
    const uint8_t s1l = (uint8_t)I[A.st_l + s1];
    switch (t.t) {
      case TT_L_L: node[t.l] = fr; push(t.k, t.l, ST_L, s1); break;
      case TT_O_O: node[t.l] = fr; rss[t.l] = 'O'; push(0, t.l, ST_O, s1); break;
      case TT_2_2: node[t.l] = fr; rss[t.l] = 'M'; push(t.k, t.l, ST_2, s1); break;
      case TT_E_H: fill_letters(rss, f.i, f.j - f.i, 3); push(t.k, t.l, ST_L, f.s); break;
      case TT_E_M: case TT_M_B: case TT_2_P: case TT_1_2: case TT_1_B: push(t.k, t.l, t.e1, f.s); break;
      case TT_P_E: case TT_P_P:
        node[f.i] = s1l; rss[f.i] = 'L'; node[t.l] = fr; rss[t.l] = 'R';
        push(t.k, t.l, t.e1, s1);
        break;
      case TT_O_OP:
        push(t.k, t.l, ST_P, s1);
        push(0, t.k, ST_O, t.s2);
        break;
      case TT_E_P: {
        const int n1 = f.j - t.l, n2 = t.k - f.i;
        if (0 == n1) fill_letters(rss, f.i, n2, 4);
        else if (0 == n2) fill_letters(rss, t.l, n1, 4);
        else { fill_letters(rss, f.i, n2, 5); fill_letters(rss, t.l, n1, 5); }
        push(t.l, f.j, ST_L, t.s3);
        push(f.i, t.k, ST_L, t.s2);
        push(t.k, t.l, ST_P, s1);
        break;
      }
      case TT_B_12:
        push(t.l, f.j, ST_2, t.s2);
        push(f.i, t.l, ST_1, s1);
        break;
      case TT_M_M: node[f.i] = s1l; rss[f.i] = 'M'; push(t.k, t.l, ST_M, s1); break;
      default: return SAMPLE_REFUSED;
    }
  }
  return SAMPLE_OK;
}

}  // namespace elemdp
