// helix_rules.h -- helix posteriors under the motif model, host / device.
//
// H(i, d, k): the probability that the k cells (i + t, d - 2 t), t = 0 .. k-1, are all pairs -- a run of k directly stacked pairs whose
// outermost pair is the cell [i, i + d) --, over the ensemble of the scan's first sum pass (terminals ari and nasi, Z = Z(ari, nasi):
// the ensemble of pair_rules.h and stem_rules.h), from its inside and outside tables.  Two pairs (i, j) and (i + 1, j - 1) of one
// derivation are joined by rule 1b alone (a rule-6c item holds at least one unpaired base), so the event is a path of k - 1 pair
// transitions along rule 1b:
//
//   v_0(s)   = out(P, i, d, s)
//   v_t(sp)  = sum over the pair transitions (s -> sp, tf), the reverse pair list of sp in list order:
//                 v_{t-1}(s) wp(s, sp, tf, i + t - 1, j - t) xst(s, cell(i + t - 1, d - 2 (t - 1)))
//              under pair_ok(i + t, d - 2 t) and d - 2 t >= 2
//   H(i, d, k) = clamp01( sum_s v_{k-1}(s) in(P, i + k - 1, d - 2 (k - 1), s) / Z )
//
// the k-step form of the 1b term of stem_rules.h, as access_rules.h is the w-step form of the emissions of node_rules.h.  H(., 1) is
// the P of pair_rules.h, H is non-increasing in k and H(i, d, k) <= H(i + 1, d - 2, k - 1), wherever the tables' inside and outside
// agree.  Nothing is renormalised.
//
// A chain starts at a kept cell and is walked once: every step gives the value of one more length.  It ends where k reaches the
// bound, where the inner cell is not kept, where the vector dies, or -- min_prob > 0 -- where H(k) < min_prob: H is non-increasing
// and smaller entries are not listed, so that pruning is exact.  Liveness is decided before every load, by control flow, never by a
// multiply; a cell that is not kept is never read.  The scaled-linear step weights carry the per-base scale (lw_pair), so a product
// of steps stays in the tables' scale; the log-space form propagates the vector in logarithms.  The lanes of a chain are a policy
// (access_rules.h): OneLane -- the CPU driver and the log-space form -- and the 64 lanes of a wave in helix_kernels.hip, lane = state,
// states beyond 64 strided over the lanes, both vectors in LDS.  The vector never lives in a per-lane array.  Every sum has a fixed
// order (list order; over the lanes a fixed tree), so a result is a function of the tables' bits.
#pragma once
#include "access_rules.h"

namespace elemdp {

constexpr int kHelixMaxLen = 32;   // ELEMDP_HELIX_MAX_LEN

struct HelixLin : NodeLin {
  ELEMDP_HD explicit HelixLin(double invZ_) : NodeLin(invZ_) {}
  ELEMDP_HD double zero() const { return 0.; }
  ELEMDP_HD double add(double a, double b) const { return a + b; }
};
struct HelixLog : NodeLog {
  ELEMDP_HD explicit HelixLog(double lnZ_) : NodeLog(lnZ_) {}
  ELEMDP_HD double zero() const { return ELEMDP_NEG_INF; }
  ELEMDP_HD double add(double a, double b) const { return lse2(a, b); }
};

// lane 0's value to every lane of the policy (a wave policy brings its own overload)
ELEMDP_HD double helix_first(const OneLane&, double v) { return v; }

struct HelixRun {
  int n;         // lengths 1 .. n were reached (and, with min_prob > 0, have H >= min_prob)
  double last;   // H(i, d, n); 0 where n = 0
};

// The chain of the kept cell [i, i + d), d >= 2 (the caller checked pair_ok(i, d)): H[k - 1] = H(i, d, k) for k = 1 .. n (H null:
// not stored), n <= kmax.  v0, v1: S entries each.  Every lane returns the same record.
template <class F, class Ln>
ELEMDP_HD HelixRun helix_chain(const F& f, const Ln& ln, const ModelView& m, const SeqView& q, const TableView& in, const TableView& out,
                               int i, int d, int kmax, double min_prob, double* v0, double* v1, double* H) {
  const AutomatonLayout& A = m.lay;
  const int32_t* I = m.ints;
  const int S = A.S;
  HelixRun r{0, 0.};
  if (!acc_load(f, ln, v0, S, [&](int s) { return f.ld(out, ST_P, d, i, s); })) return r;
  for (int k = 1;; ++k) {
    const int ik = i + k - 1, dk = d - 2 * (k - 1);   // the innermost cell of length k: kept
    const double o0 = ln.lane() < S ? f.ld(in, ST_P, dk, ik, ln.lane()) : f.zero();
    double h = acc_dot(f, ln, v0, S, o0, [&](int s) { return f.ld(in, ST_P, dk, ik, s); });
    h = helix_first(ln, ctx_clamp(h));
    if (min_prob > 0. && h < min_prob) return r;
    if (H && ln.lane() == 0) H[k - 1] = h;
    r.n = k; r.last = h;
    if (k >= kmax || dk - 2 < 2 || !q.pair_ok(ik + 1, dk - 2)) return r;
    const int c = q.cell(ik, dk);
    const bool live = acc_step(f, ln, I + A.rpair_off, I + A.rpair_ent, v0, v1, S, [&](int sp, int s, int tf) {
      return f.mul(f.w_pair2(m, q, s, sp, tf, ik, ik + dk - 1), f.w_stack(m, q, s, c));
    });
    if (!live) return r;
    double* t = v0; v0 = v1; v1 = t;
  }
}

// The stem of a caller-given structure whose outermost pair is the cell [i, i + d) and which holds len pairs: the joint probability
// of the whole stem, no bound on the length, no threshold.  0 exactly where a pair of the stem is no kept cell (a span above the
// band among them) or the chain dies.
template <class F, class Ln>
ELEMDP_HD double helix_stem(const F& f, const Ln& ln, const ModelView& m, const SeqView& q, const TableView& in, const TableView& out,
                            int i, int d, int len, double* v0, double* v1) {
  if (len < 1 || d < 2 || !q.pair_ok(i, d)) return 0.;
  const HelixRun r = helix_chain(f, ln, m, q, in, out, i, d, len, 0., v0, v1, (double*)nullptr);
  return r.n == len ? r.last : 0.;
}

// where the values and the reached length of unit r of a table slot lie: rows of `mult` doubles
ELEMDP_HD size_t helix_at(int mult, size_t r, int k) { return r * (size_t)mult + (size_t)(k - 1); }
// units of a slot's scratch (host): one per cell of the largest sequence
inline size_t helix_units_cap(int Lmax, int Wmax) { return ((size_t)Lmax + 1) * ((size_t)Wmax + 1); }

}  // namespace elemdp
