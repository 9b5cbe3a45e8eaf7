// access_rules.h -- accessibility under the motif model, host / device.
//
// access(a, w): the probability that the bases a .. a+w-1 of a sequence are all unpaired, over the ensemble of the scan's first sum
// pass (terminals ari and nasi, Z = Z(ari, nasi): the ensemble of pair_rules.h, ctx_rules.h and node_rules.h), from its inside and
// outside tables.  A window [a, b), b = a + w, of unpaired bases lies in exactly one maximal unpaired stretch, and the grammar
// makes such a stretch by exactly one of four chains of single emissions; the window is unpaired iff the derivation holds the
// item in front of base a and the item behind base b-1 of one chain, joined by w emissions.  Every term is divided by Z:
//
//   T_L  loop runs (hairpin, bulge, both sides of an interior loop): every L(i, j), j > i, is made by one L <- L emission, so a run
//        that starts at i <= a and reaches b holds the item L(i, b):
//            T_L(a, w) = sum_{i <= a, b-i <= W} u(i, b-i)        u(i, d) = sum_s in(L, i, d, s) out(L, i, d, s) of ctx_rules.h
//        a sum along the column of the right end b, kept per (b, w): the sum over the spans d >= w.
//   T_O  exterior (rule 8): v <- in_o(a, .); per base p = a .. b-1 under unp[p]: v'(s) = sum_{s1 in right(s)} v(s1) wr(s, tf, p);
//            T_O = sum_s v(s) out_o(b, s)
//   T_2  tails behind a multi-loop branch (rule 3a), left end k < a fixed, b - k <= W: v <- in(2, k, a-k, .), the same emissions
//        under the guards of rule 3a at every step (unp[p], left_ok of both cells); T_2 += sum_s v(s) out(2, k, b-k, s).
//        The compact scaled-linear tables keep only the direct part of out(2); what a 2 entry takes as the right part of a
//        bifurcation lives in the pair table of the factorised rule 2, whose tail step IS rule 3a (node_rules.h).  That form adds
//        the same chain on the pair table: v <- in_A(k, a-k, .), stepped with the ap_chain transitions where the entries exist
//        (0 < dmin[k] < d), against out_A(k, b-k, .) -- the multi-step form of NodeLin::chain.  The dense log-space tables hold the
//        whole out(2) and have no pair table.
//   T_M  leading bases of a multi-loop (rule 5a), right end j > b fixed, j - a <= W: v <- in(M, b, j-b, .); per base p = b-1 down to a
//        under unp[p] and m_ok of both cells: v'(s) = sum_{sl in left(s)} v(sl) wl(sl, tf, p); T_M += sum_s v(s) out(M, a, j-a, s)
//
//   access(a, w) = clamp01(((T_L + T_O) + T_2) + T_M);  NaN where a + w > L.
//
// Every chain is walked once: from a start cell the vector is extended one base at a time, up to U = max_width steps, and every
// step gives the term of one width.  A chain of T_O and T_2 starts in front of a and serves the windows (a, 1 .. U); a chain of T_M
// and the column of T_L end behind b-1 and serve the windows (b-w, w).  So a unit of work is (term, position x) and writes the U
// values of row x of the term's plane: T_O, T_2 by the window's start, T_L, T_M by its end.  A start vector without a live entry
// is skipped before any step, and a chain ends where its vector dies.  Within a unit the order is fixed: start cells by
// increasing span, the direct chain of a cell before its pair-table chain, widths in increasing order.
//
// One template for both forms (AccLin / AccLog, as CtxLin / CtxLog, NodeLin / NodeLog).  The scaled-linear weights lw_right /
// lw_left carry the per-base scale, so a product of steps across cells stays in the tables' scale as the one-step products of
// node_rules.h do; the log-space form propagates the vector in logarithms.  Liveness is decided before every load, by control
// flow, never by a multiply.  With max_iloop < 30 the outside pass enumerates interior loops the inside pass does not (SURVEY §7
// quirk ii); out(L) carries that and T_L follows the tables as ctx_rules.h does.
//
// The lanes that work on one unit are a policy (Ln): OneLane here -- the CPU driver and the log-space form, one thread per unit --
// and the 64 lanes of a wave in access_kernels.hip, lane = state, the vector in LDS.  The vector never lives in a per-lane array.
#pragma once
#include "node_rules.h"

namespace elemdp {

constexpr int kAccessMaxWidth = 64;
enum AccessTerm : int { ACC_L = 0, ACC_O = 1, ACC_2 = 2, ACC_M = 3, ACC_TERMS = 4 };

struct AccLin : NodeLin {
  enum { pair_table = 1 };
  // p0: the position of entry 0 of q.seq / q.ews where a unit's bases are staged (access_kernels.hip); 0: the whole sequence
  int p0;
  ELEMDP_HD explicit AccLin(double invZ_, int p0_ = 0) : NodeLin(invZ_), p0(p0_) {}
  ELEMDP_HD double w_emit(const ModelView& m, const SeqView& q, int par, int tf, int pos) const { return lw_right(m, q, par, tf, pos - p0); }
  ELEMDP_HD double w_left(const ModelView& m, const SeqView& q, int ch, int tf, int pos) const { return lw_left(m, q, ch, tf, pos - p0); }
  ELEMDP_HD double zero() const { return 0.; }
  ELEMDP_HD double add(double a, double b) const { return a + b; }
  ELEMDP_HD double ld_a(const TableView& T, int d, int i, int p) const { return T.a(d, i, p); }
};
struct AccLog : NodeLog {
  enum { pair_table = 0 };
  ELEMDP_HD explicit AccLog(double lnZ_) : NodeLog(lnZ_) {}
  ELEMDP_HD double zero() const { return ELEMDP_NEG_INF; }
  ELEMDP_HD double add(double a, double b) const { return lse2(a, b); }
  ELEMDP_HD double ld_a(const TableView&, int, int, int) const { return ELEMDP_NEG_INF; }
};

// one lane per unit
struct OneLane {
  ELEMDP_HD int lane() const { return 0; }
  ELEMDP_HD int n() const { return 1; }
  ELEMDP_HD void sync() const {}
  ELEMDP_HD double sum(double v) const { return v; }     // over the lanes, to lane 0
  ELEMDP_HD bool any(bool b) const { return b; }
  ELEMDP_HD double scan(double v) const { return v; }    // inclusive, in lane order
  ELEMDP_HD double last(double v) const { return v; }    // the last lane's value, to every lane
  template <class P> ELEMDP_HD uint64_t mask(int n, P pred) const {   // bit w = pred(w), w < n <= 64
    uint64_t b = 0;
    for (int w = 0; w < n; ++w) b |= (uint64_t)(pred(w) ? 1 : 0) << w;
    return b;
  }
};

// v[0 .. n) <- ld(.); false: no live entry
template <class F, class Ln, class Ld>
ELEMDP_HD bool acc_load(const F& f, const Ln& ln, double* v, int n, Ld ld) {
  bool live = false;
  for (int s = ln.lane(); s < n; s += ln.n()) {
    const double x = ld(s);
    v[s] = x;
    live = live || !f.dead(x);
  }
  ln.sync();
  return ln.any(live);
}
// v1(s) = sum over the list of s (child c, tau flag) of v0(c) wt(s, c, flag), entries in list order; false: v1 is dead
template <class F, class Ln, class Wt>
ELEMDP_HD bool acc_step(const F& f, const Ln& ln, const int32_t* off, const int32_t* ent, const double* v0, double* v1, int n, Wt wt) {
  bool live = false;
  for (int s = ln.lane(); s < n; s += ln.n()) {
    double a = f.zero();
    for (int t = off[s]; t < off[s + 1]; ++t) {
      const double x = v0[ent[2 * t]];
      if (f.dead(x)) continue;
      a = f.add(a, f.mul(x, wt(s, ent[2 * t], ent[2 * t + 1])));
    }
    v1[s] = a;
    live = live || !f.dead(a);
  }
  ln.sync();
  return ln.any(live);
}
// sum_s v(s) ld(s) / Z, states in increasing order per lane (valid in lane 0); o0: ld of the lane's first entry, loaded ahead
template <class F, class Ln, class Ld>
ELEMDP_HD double acc_dot(const F& f, const Ln& ln, const double* v, int n, double o0, Ld ld) {
  double a = f.zero();
  for (int s = ln.lane(); s < n; s += ln.n()) {
    const double x = v[s];
    if (f.dead(x)) continue;
    a = f.add(a, f.mul(x, s == ln.lane() ? o0 : ld(s)));
  }
  return ln.sum(f.post(a));
}
// one chain from the live start vector v0: widths 1 .. U while ok(w); dst[w-1] += the term of width w.  The outside entry of a
// step is loaded before the step (the cell is live by ok(w)): its latency runs next to the step's.
template <class F, class Ln, class Ok, class Wt, class Out>
ELEMDP_HD void acc_walk(const F& f, const Ln& ln, const int32_t* off, const int32_t* ent, double* v0, double* v1, int n, int U, Ok ok,
                        Wt wt, Out out, double* dst) {
  for (int w = 1; w <= U; ++w) {
    if (!ok(w)) return;
    const double o0 = ln.lane() < n ? out(w, ln.lane()) : f.zero();
    if (!acc_step(f, ln, off, ent, v0, v1, n, [&](int s, int c, int tf) { return wt(w, s, c, tf); })) return;
    double* t = v0; v0 = v1; v1 = t;
    const double term = acc_dot(f, ln, v0, n, o0, [&](int s) { return out(w, s); });
    if (ln.lane() == 0) dst[w - 1] += term;
  }
}
template <class Ln>
ELEMDP_HD void acc_clear(const Ln& ln, double* dst, int U) {
  if (ln.lane() == 0)
    for (int w = 0; w < U; ++w) dst[w] = 0.;
}

// T_L by the window's end b: dst[w-1] = sum_{d = w .. min(W, b)} u(b-d, d).  The spans in decreasing order, a block of one span per
// lane at a time: the sum over the larger spans so far plus the block's inclusive scan.
template <class F, class Ln>
ELEMDP_HD void access_loop(const F& f, const Ln& ln, const ModelView& m, const SeqView& q, const TableView& in, const TableView& out,
                           int b, int U, double* dst) {
  const AutomatonLayout& A = m.lay;
  const int32_t* I = m.ints;
  const int dmax = (b < 1 || b > q.L) ? 0 : (q.W < b ? q.W : b);
  for (int w = dmax + 1 + ln.lane(); w <= U; w += ln.n()) dst[w - 1] = 0.;
  double run = 0.;
  for (int hi = dmax; hi >= 1; hi -= ln.n()) {
    const int d = hi - ln.lane();
    double u = 0.;
    if (d >= 1)
      for (int s = 0; s < A.S; ++s) {
        if (!I[A.st_is_loop + s]) continue;
        const double inL = f.ld(in, ST_L, d, b - d, s);
        if (f.dead(inL)) continue;
        u += f.post(f.mul(inL, f.ld(out, ST_L, d, b - d, s)));
      }
    const double inc = ln.scan(u);
    if (d >= 1 && d <= U) dst[d - 1] = run + inc;
    run += ln.last(inc);
  }
}

// T_O by the window's start a
template <class F, class Ln>
ELEMDP_HD void access_exterior(const F& f, const Ln& ln, const ModelView& m, const SeqView& q, const TableView& in, const TableView& out,
                               int a, int U, double* v0, double* v1, double* dst) {
  const AutomatonLayout& A = m.lay;
  const int32_t* I = m.ints;
  acc_clear(ln, dst, U);
  if (a >= q.L) return;
  const uint64_t unp = ln.mask(U, [&](int w) { return a + w < q.L && q.unp[a + w] != 0; });   // (bit w-1: base a + w - 1 may be unpaired)
  if (!acc_load(f, ln, v0, A.S, [&](int s) { return in.o(a, s); })) return;
  acc_walk(f, ln, I + A.right_off, I + A.right_ent, v0, v1, A.S, U,
           [&](int w) { return ((unp >> (w - 1)) & 1) != 0; },
           [&](int w, int s, int, int tf) { return f.w_emit(m, q, s, tf, a + w - 1); },
           [&](int w, int s) { return out.o(a + w, s); }, dst);
}

// T_2 by the window's start a: the left ends k = a - d0, d0 = 1, 2, ..; per k the chain on plane 2, then the chain on the pair table
template <class F, class Ln>
ELEMDP_HD void access_tails(const F& f, const Ln& ln, const ModelView& m, const SeqView& q, const TableView& in, const TableView& out,
                            int a, int U, double* v0, double* v1, double* dst) {
  const AutomatonLayout& A = m.lay;
  const int32_t* I = m.ints;
  acc_clear(ln, dst, U);
  if (a < 1 || a >= q.L) return;
  const uint64_t unp = ln.mask(U, [&](int w) { return a + w < q.L && q.unp[a + w] != 0; });
  if (!(unp & 1)) return;
  for (int d0 = 1; d0 < q.W && d0 <= a; ++d0) {
    const int k = a - d0;
    const int dm = q.dmin[k];
    if (dm <= 0) continue;
    // (a cell (k, d), d > d0, is left_ok with (k, d0) as long as it lies in the band and the sequence)
    auto ok = [&](int w) { return d0 + w <= q.W && ((unp >> (w - 1)) & 1) != 0; };
    if (d0 >= dm && acc_load(f, ln, v0, A.S, [&](int s) { return f.ld(in, ST_2, d0, k, s); }))
      acc_walk(f, ln, I + A.right_off, I + A.right_ent, v0, v1, A.S, U, ok,
               [&](int w, int s, int, int tf) { return f.w_emit(m, q, s, tf, a + w - 1); },
               [&](int w, int s) { return f.ld(out, ST_2, d0 + w, k, s); }, dst);
    if (F::pair_table && d0 > dm && acc_load(f, ln, v0, A.n_ap, [&](int p) { return f.ld_a(in, d0, k, p); }))
      acc_walk(f, ln, I + A.ap_chain_off, I + A.ap_chain_ent, v0, v1, A.n_ap, U, ok,
               [&](int w, int p, int, int tf) { return f.w_emit(m, q, I[A.ap_t + p], tf, a + w - 1); },
               [&](int w, int p) { return f.ld_a(out, d0 + w, k, p); }, dst);
  }
}

// T_M by the window's end b: the right ends j = b + d0, d0 = m_min, ..
template <class F, class Ln>
ELEMDP_HD void access_leads(const F& f, const Ln& ln, const ModelView& m, const SeqView& q, const TableView& in, const TableView& out,
                            int b, int U, double* v0, double* v1, double* dst) {
  const AutomatonLayout& A = m.lay;
  const int32_t* I = m.ints;
  acc_clear(ln, dst, U);
  if (b < 2 || b >= q.L) return;
  const uint64_t unp = ln.mask(U, [&](int w) { return b - 1 - w >= 0 && q.unp[b - 1 - w] != 0; });   // (bit w-1: base b - w)
  if (!(unp & 1)) return;
  for (int d0 = m.m_min; d0 < q.W && b + d0 < q.L; ++d0) {
    if (!m_ok(m, q, b, d0)) continue;
    if (!acc_load(f, ln, v0, A.S, [&](int s) { return f.ld(in, ST_M, d0, b, s); })) continue;
    acc_walk(f, ln, I + A.left_off, I + A.left_ent, v0, v1, A.S, U,
             [&](int w) { return m_ok(m, q, b - w, d0 + w) && ((unp >> (w - 1)) & 1) != 0; },
             [&](int w, int, int sl, int tf) { return f.w_left(m, q, sl, tf, b - w); },
             [&](int w, int s) { return f.ld(out, ST_M, d0 + w, b - w, s); }, dst);
  }
}

// the unit (term, x), 0 <= x <= L: the U values of row x of the term's plane; v0, v1: S entries each, max(S, n_ap) where the form
// has a pair table
template <class F, class Ln>
ELEMDP_HD void access_unit(const F& f, const Ln& ln, const ModelView& m, const SeqView& q, const TableView& in, const TableView& out,
                           int term, int x, int U, double* v0, double* v1, double* dst) {
  if (term == ACC_L) access_loop(f, ln, m, q, in, out, x, U, dst);
  else if (term == ACC_O) access_exterior(f, ln, m, q, in, out, x, U, v0, v1, dst);
  else if (term == ACC_2) access_tails(f, ln, m, q, in, out, x, U, v0, v1, dst);
  else access_leads(f, ln, m, q, in, out, x, U, v0, v1, dst);
}
// a sequence without any parse: the exterior plane is 1
ELEMDP_HD void access_unit_no_parse(int term, int U, double* dst) {
  for (int w = 0; w < U; ++w) dst[w] = term == ACC_O ? 1. : 0.;
}

// access(a, w) from the four planes T + term * plane, rows of U; the terms in a fixed order
ELEMDP_HD double access_value(const double* T, size_t plane, int L, int U, int a, int w) {
  if (a + w > L) return __builtin_nan("");
  const size_t s = (size_t)a * U + (w - 1), e = (size_t)(a + w) * U + (w - 1);
  return ctx_clamp(((T[ACC_L * plane + e] + T[ACC_O * plane + s]) + T[ACC_2 * plane + s]) + T[ACC_M * plane + e]);
}
// no secondary structure in the model (ELEMDP_NO_RSS): every valid window is unpaired
ELEMDP_HD double access_value_no_rss(int L, int a, int w) { return a + w > L ? __builtin_nan("") : 1.; }

}  // namespace elemdp
