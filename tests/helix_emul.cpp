// Test-only CPU driver of the helix posteriors: the product's rules of the scan's first sum pass on the CPU, as
// emu_scan_seq_lin (scaled-linear, compact tables) and emu_scan_seq (log space, dense tables) run them, then the chain of
// helix_rules.h on the finished tables, one lane per unit.  Not part of the product.
#include "emul/emul.cpp"

#include "../rnaelem_amd/csrc/helix_rules.h"

namespace {

struct HelixJob {
  int max_len; double min_prob;
  double* H;        // max_len (W+1) (L+1) doubles, H[((k - 1) (W+1) + d) (L+1) + i]; 0 where the chain did not reach length k
  int n_stems; const int32_t* s_i; const int32_t* s_d; const int32_t* s_len; double* s_p;
};

// live false: no parse at all, or a model without secondary structure (the tables are not read)
template <class F>
void helix_all(const F& f, const ModelView& m, const SeqView& q, const TableView& in, const TableView& out, bool live, const HelixJob& job) {
  const int L = q.L, W = q.W, S = m.lay.S;
  std::vector<double> v0(S), v1(S), row(job.max_len);
  const OneLane ln;
  for (size_t t = 0; t < (size_t)job.max_len * (W + 1) * (L + 1); ++t) job.H[t] = 0.;
  for (int t = 0; t < job.n_stems; ++t) job.s_p[t] = 0.;
  if (!live) return;
  for (int i = 0; i <= L; ++i)
    for (int d = 2; d <= W && i + d <= L; ++d) {
      if (!q.pair_ok(i, d)) continue;
      const HelixRun r = helix_chain(f, ln, m, q, in, out, i, d, job.max_len, job.min_prob, v0.data(), v1.data(), row.data());
      for (int k = 1; k <= r.n; ++k) job.H[((size_t)(k - 1) * (W + 1) + d) * (L + 1) + i] = row[k - 1];
    }
  for (int t = 0; t < job.n_stems; ++t)
    job.s_p[t] = helix_stem(f, ln, m, q, in, out, job.s_i[t], job.s_d[t], job.s_len[t], v0.data(), v1.data());
}

void softmax_theta(const Emu& E, const double* x, std::vector<double>& theta) {
  if (!(E.flags & F_SOFTMAX)) return;
  for (int r = 0; r < E.au->n_rows(); ++r) {
    double tot = NEG;
    for (int c = 0; c < E.au->row_width(r); ++c) tot = lse2(tot, x[E.au->row_offset(r) + c]);
    for (int c = 0; c < E.au->row_width(r); ++c) theta[E.au->row_offset(r) + c] = x[E.au->row_offset(r) + c] - tot;
  }
}

void helix_log(Emu& E, const double* x, const uint8_t* seq, int L, const uint8_t* qual, const HelixJob& job) {
  const int nt = E.au->n_theta();
  std::vector<double> theta(x, x + nt);
  softmax_theta(E, x, theta);
  ModelView m = make_view(E.lay, E.ints, theta.data(), x[nt], x[nt + 1], std::log(E.tau), E.flags & F_NO_PRF, E.flags & F_NO_TURN);
  HostPlan P;
  prepare(E, P, seq, L, qual, nullptr);
  SeqView q = P.view();
  const int S = m.lay.S;
  Tab in(L, P.W, S), out(L, P.W, S);
  std::vector<double> Pys(L, NEG), Pyi(L, NEG), en(nt + 1, 0.);
  double eh[2] = {0, 0};
  const Constraint c0{-1, -1, 0};
  run_inside<false>(m, q, in, c0);
  const double ZL = part_func(m, in.v, true, true);
  CpuSink s1{en.data(), eh, {Pys.data(), Pyi.data(), nullptr}};
  run_outside<OUT_SCAN>(m, q, in, out, ZL, c0, s1, true, true);
  helix_all(HelixLog(ZL), m, q, in.v, out.v, ZL > NEG && ZL < HUGE_VAL && !(E.flags & F_NO_RSS), job);
}

// 0: done in the scaled-linear form; 1: Z left the double range (or is 0), nothing written
int helix_lin(Emu& E, const double* x, const uint8_t* seq, int L, const uint8_t* qual, const HelixJob& job) {
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
  LinTab in(L, P.W, m.lay, E.ints.data()), out(L, P.W, m.lay, E.ints.data());   // (NaN-filled: a dead read shows up)
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
  const double Z = lin_part(m, in.v, true, true);
  if (!(Z > 0. && Z < HUGE_VAL)) return 1;
  std::vector<double> Pys(L, 0.), Pyi(L, 0.), en(nt + 1, 0.);
  double eh[2] = {0, 0};
  CpuLinSink s1{en.data(), eh, {Pys.data(), Pyi.data(), nullptr}};
  LinOutCtx<CpuLinSink> xo{m, q, in.v, out.v, 1. / Z, s1, c0};
  out.v.o(L, m.lay.s00) = 1.; out.v.o(L, m.lay.s0m1) = 1.; out.v.o(L, m.lay.s0m2) = 1.;
  for (int i = L - 1; i >= 0; --i) for (int s = 0; s < S; ++s) lin_outside_ext_target<OUT_SCAN>(xo, i, s);
  if (fast) fast_rule7(m, q, in.v, out.v);
  for (int d = q.W; d >= 0; --d) for (int i = 0; i + d <= L; ++i) {
    if (fast) { fast_outside_cell<OUT_SCAN>(xo, (LinOutCtx<CpuLinSink>*)nullptr, d, i, -1); continue; }
    for (int s = 0; s < S; ++s) lin_outside_target<OUT_SCAN>(xo, d, i, s);
    lin_outside_cell_pairs<OUT_SCAN>(xo, d, i);
  }
  helix_all(HelixLin(1. / Z), m, q, in.v, out.v, !(E.flags & F_NO_RSS), job);
  return 0;
}

}  // namespace

extern "C" {

// the span W the plan of a sequence of length L has (the row length of H)
int emu_helix_span(void* h, const uint8_t* seq, int L, const uint8_t* qual) {
  try {
    Emu& E = *(Emu*)h;
    HostPlan P;
    prepare(E, P, seq, L, qual, nullptr);
    return P.W;
  } catch (std::exception& e) { g_err = e.what(); return -1; }
}

// H: max_len (W+1) (L+1) doubles, H[((k - 1) (W+1) + d) (L+1) + i], 0 where the chain of cell (i, d) did not reach length k (with
// min_prob > 0: or fell below it); the n_stems stems (s_i, s_d, s_len) -> s_p.  form 0: the scaled-linear form, and the log-space
// form where Z leaves the double range or the sequence has no parse (as the engine hands such a sequence on); form 1: the
// log-space form.  Returns the form that wrote H, or -1 with emu_last_error.
int emu_helix_seq(void* h, const double* x, const uint8_t* seq, int L, const uint8_t* qual, int form, int max_len, double min_prob,
                  double* H, int n_stems, const int32_t* s_i, const int32_t* s_d, const int32_t* s_len, double* s_p) {
  try {
    Emu& E = *(Emu*)h;
    if (max_len < 1) throw std::runtime_error("max_len must be >= 1");
    const HelixJob job{max_len, min_prob, H, n_stems, s_i, s_d, s_len, s_p};
    if (form == 0 && helix_lin(E, x, seq, L, qual, job) == 0) return 0;
    helix_log(E, x, seq, L, qual, job);
    return 1;
  } catch (std::exception& e) { g_err = e.what(); return -1; }
}

}  // extern "C"
