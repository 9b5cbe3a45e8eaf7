// Test-only CPU driver of the motif-conditional pair posteriors: the product's rules of the scan's inside sweep on the
// CPU, then one outside sweep per world -- seeded with the ari terminals alone, then with the nasi terminal alone -- as
// emu_scan_seq_lin (scaled-linear, compact tables) and emu_scan_seq (log space, dense tables) run them, and the rule of
// cond_rules.h on the finished tables.  Not part of the product.
#include "emul/emul.cpp"

#include "../rnaelem_amd/csrc/cond_rules.h"

namespace {

// what the driver hands back for one sequence: P of both worlds ([i][d], rows of W+1), both unpaired vectors, exist_prob, shift
struct CondOutput { double* P[2]; double* unp[2]; double* exist; double* shift; };

// the per-sequence pass of k_cond_seq: unpaired of both worlds, exist_prob, shift with its rows in increasing i
void cond_finish(const CondZ& z, const SeqView& q, const CondOutput& o) {
  const int L = q.L, W = q.W;
  for (int p = 0; p < L; ++p)
    for (int w = 0; w < 2; ++w) o.unp[w][p] = pair_unpaired(o.P[w], q.okbits, L, W, p);
  double acc = 0.;
  for (int i = 0; i <= L; ++i) acc += cond_shift_row(o.P[0], o.P[1], q.okbits, W, i, std::min(W, L - i));
  *o.exist = z.exist();
  *o.shift = (z.empty(COND_MOTIF) || z.empty(COND_NONE)) ? std::numeric_limits<double>::quiet_NaN() : acc;
}

// the pair reduction of one world: R = PairLin over TableView::ld, or PairLog over TableView::at
template <class R, class Ld>
void cond_cells(const R& r, Ld ld, bool live, const ModelView& m, const SeqView& q, double* P) {
  const int L = q.L, W = q.W;
  for (int i = 0; i <= L; ++i)
    for (int d = 0; d <= W; ++d) {
      double acc = 0.;
      if (live && i + d <= L && q.pair_ok(i, d))
        for (int s = 0; s < m.lay.S; ++s)
          if (s != m.lay.shadow) acc += r.term(ld(0, d, i, s), ld(1, d, i, s));
      P[(size_t)i * (W + 1) + d] = live ? r.finish(acc) : 0.;
    }
}

void softmax_theta(const Emu& E, const double* x, std::vector<double>& theta) {
  if (!(E.flags & F_SOFTMAX)) return;
  for (int r = 0; r < E.au->n_rows(); ++r) {
    double tot = NEG;
    for (int c = 0; c < E.au->row_width(r); ++c) tot = lse2(tot, x[E.au->row_offset(r) + c]);
    for (int c = 0; c < E.au->row_width(r); ++c) theta[E.au->row_offset(r) + c] = x[E.au->row_offset(r) + c] - tot;
  }
}

void cond_log(Emu& E, const double* x, const uint8_t* seq, int L, const uint8_t* qual, const CondOutput& o) {
  const int nt = E.au->n_theta();
  std::vector<double> theta(x, x + nt);
  softmax_theta(E, x, theta);
  ModelView m = make_view(E.lay, E.ints, theta.data(), x[nt], x[nt + 1], std::log(E.tau), E.flags & F_NO_PRF, E.flags & F_NO_TURN);
  HostPlan P;
  prepare(E, P, seq, L, qual, nullptr);
  SeqView q = P.view();
  const int S = m.lay.S;
  Tab in(L, P.W, S);
  const Constraint c0{-1, -1, 0};
  run_inside<false>(m, q, in, c0);
  const CondZ z{part_func(m, in.v, true, true), part_func(m, in.v, true, false), part_func(m, in.v, false, true), true};
  for (int w = 0; w < 2; ++w) {
    const double Zw = z.of(w);
    const bool live = Zw > NEG && Zw < HUGE_VAL;
    const bool rss = !(E.flags & F_NO_RSS);   // (a model without secondary structure keeps no pair: plane P is no pair posterior there)
    Tab out(L, P.W, S);
    if (live) {
      std::vector<double> Pys(L, NEG), Pyi(L, NEG), en(nt + 1, 0.);
      double eh[2] = {0, 0};
      CpuSink s1{en.data(), eh, {Pys.data(), Pyi.data(), nullptr}};
      run_outside<OUT_SCAN>(m, q, in, out, Zw, c0, s1, w == COND_MOTIF, w == COND_NONE);
    }
    cond_cells(PairLog{Zw}, [&](int side, int d, int i, int s) { return (side ? out.v : in.v).at(ST_P, d, i, s); }, live && rss, m, q, o.P[w]);
  }
  cond_finish(z, q, o);
}

// 0: done in the scaled-linear form; 1: one of the three Z is non-zero and left the double range, nothing written
int cond_lin(Emu& E, const double* x, const uint8_t* seq, int L, const uint8_t* qual, const CondOutput& o) {
  const int nt = E.au->n_theta();
  std::vector<double> theta(x, x + nt);
  softmax_theta(E, x, theta);
  const bool no_prf = E.flags & F_NO_PRF;
  std::vector<double> lin;
  make_lin_params(E.lay, E.ints.data(), theta.data(), E.tau, no_prf, &lin);
  ModelView m = make_view(E.lay, E.ints, theta.data(), x[nt], x[nt + 1], std::log(E.tau), no_prf, E.flags & F_NO_TURN);
  m.lin = lin.data();
  HostPlan P;
  prepare(E, P, seq, L, qual, nullptr);
  SeqView q = P.view();
  const int S = m.lay.S;
  const size_t nc = (size_t)(L + 1) * (P.W + 1), ni = P.items.size();
  std::vector<double> ews(L + 1), xwc(10 * nc), xwi(2 * ni + 1);
  for (int p = 0; p <= L; ++p) ews[p] = std::exp(P.ws[p]);
  const double* terms[5] = {P.e_stack.data(), P.e_ext.data(), P.e_ml.data(), P.e_close.data(), P.e_hp.data()};
  for (int k = 0; k < 2; ++k) {
    for (int t = 0; t < 5; ++t)
      for (size_t c = 0; c < nc; ++c) xwc[(size_t)(k * 5 + t) * nc + c] = lin_weight(m.lambda[k], terms[t][c]);
    for (size_t n = 0; n < ni; ++n) xwi[(size_t)k * ni + n] = lin_weight(m.lambda[k], P.items[n].tsc);
  }
  q.ews = ews.data(); q.xwc = xwc.data(); q.xwc_stride = nc; q.xwi = xwi.data(); q.xwi_stride = ni;
  LinTab in(L, P.W, m.lay, E.ints.data());   // (NaN-filled: a dead read shows up)
  const bool fast = E.fast && m.lay.fp_ok;
  const Constraint c0{-1, -1, 0};
  for (int d = 0; d <= q.W; ++d)
    for (int i = 0; i + d <= q.L; ++i) {
      if (fast) { fast_inside_cell<false>(m, q, in.v, d, i, c0); continue; }
      lin_inside_cell_pairs<false>(m, q, in.v, d, i, c0);
      for (int s = 0; s < S; ++s) lin_inside_target<false>(m, q, in.v, d, i, s, c0);
    }
  for (int s = 0; s < S; ++s) in.v.o(0, s) = (s == m.lay.s00) ? 1. : 0.;
  for (int j = 1; j <= L; ++j)
    for (int s = 0; s < S; ++s) lin_inside_ext_target<false>(m, q, in.v, j, s, c0);
  const CondZ z{lin_part(m, in.v, true, true), lin_part(m, in.v, true, false), lin_part(m, in.v, false, true), false};
  for (double Z : {z.zo, z.za, z.zn})
    if (Z != 0. && !(Z > 0. && Z < HUGE_VAL)) return 1;
  for (int w = 0; w < 2; ++w) {
    const bool live = !z.empty(w);
    // (a fresh NaN-filled outside table per world: an entry the nasi sweep does not write cannot pass for one the ari sweep left)
    LinTab out(L, P.W, m.lay, E.ints.data());
    if (live) {
      std::vector<double> Pys(L, 0.), Pyi(L, 0.), en(nt + 1, 0.);
      double eh[2] = {0, 0};
      CpuLinSink s1{en.data(), eh, {Pys.data(), Pyi.data(), nullptr}};
      LinOutCtx<CpuLinSink> xo{m, q, in.v, out.v, 1. / z.of(w), s1, c0};
      if (w == COND_MOTIF) { out.v.o(L, m.lay.s0m1) = 1.; out.v.o(L, m.lay.s0m2) = 1.; }
      else out.v.o(L, m.lay.s00) = 1.;
      for (int i = L - 1; i >= 0; --i) for (int s = 0; s < S; ++s) lin_outside_ext_target<OUT_SCAN>(xo, i, s);
      if (fast) fast_rule7(m, q, in.v, out.v);
      for (int d = q.W; d >= 0; --d) for (int i = 0; i + d <= L; ++i) {
        if (fast) { fast_outside_cell<OUT_SCAN>(xo, (LinOutCtx<CpuLinSink>*)nullptr, d, i, -1); continue; }
        for (int s = 0; s < S; ++s) lin_outside_target<OUT_SCAN>(xo, d, i, s);
        lin_outside_cell_pairs<OUT_SCAN>(xo, d, i);
      }
    }
    cond_cells(PairLin{live ? 1. / z.of(w) : 0.}, [&](int side, int d, int i, int s) { return (side ? out.v : in.v).ld(ST_P, d, i, s); }, live && !(E.flags & F_NO_RSS), m, q, o.P[w]);
  }
  cond_finish(z, q, o);
  return 0;
}

}  // namespace

extern "C" {

// P_motif, P_none: (L+1) * (W+1) doubles each ([i][d], W = min(L, max_span)); unp_motif, unp_none: L doubles; out2: exist_prob,
// shift.  form 0: the scaled-linear form, and the log-space form where one of the three Z is non-zero and leaves the double
// range (as the engine hands such a sequence on); form 1: the log-space form.  Returns the form that wrote the result, or -1
// with emu_last_error.
int emu_cond_seq(void* h, const double* x, const uint8_t* seq, int L, const uint8_t* qual, int form, double* P_motif, double* P_none,
                 double* unp_motif, double* unp_none, double* out2) {
  try {
    Emu& E = *(Emu*)h;
    const CondOutput o{{P_motif, P_none}, {unp_motif, unp_none}, out2, out2 + 1};
    if (form == 0 && cond_lin(E, x, seq, L, qual, o) == 0) return 0;
    cond_log(E, x, seq, L, qual, o);
    return 1;
  } catch (std::exception& e) { g_err = e.what(); return -1; }
}

}  // extern "C"
