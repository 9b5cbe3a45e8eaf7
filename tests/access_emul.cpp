// Test-only CPU driver of the accessibility: the product's rules of the scan's first sum pass on the CPU, as
// emu_scan_seq_lin (scaled-linear, compact tables) and emu_scan_seq (log space, dense tables) run them, then the rule of
// access_rules.h on the finished tables, one lane per unit.  Not part of the product.
#include "emul/emul.cpp"

#include "../rnaelem_amd/csrc/access_rules.h"

namespace {

// the four planes unit by unit, then every window; parse false: no parse at all; rss false: a model without secondary structure.
// terms (optional): the planes by the window's start, terms[(4 * a + term) * U + (w - 1)]
template <class F>
void access_all(const F& f, const ModelView& m, const SeqView& q, const TableView& in, const TableView& out, bool parse, bool rss, int U,
                double* access, double* terms) {
  const int L = q.L;
  const size_t plane = (size_t)(L + 1) * U;
  const int nv = std::max(m.lay.S, m.lay.n_ap);
  std::vector<double> T(ACC_TERMS * plane, 0.), v0(nv), v1(nv);
  const OneLane ln;
  if (rss)
    for (int term = 0; term < ACC_TERMS; ++term)
      for (int x = 0; x <= L; ++x) {
        double* dst = T.data() + term * plane + (size_t)x * U;
        if (parse) access_unit(f, ln, m, q, in, out, term, x, U, v0.data(), v1.data(), dst);
        else access_unit_no_parse(term, U, dst);
      }
  for (int a = 0; a < L; ++a)
    for (int w = 1; w <= U; ++w) {
      access[(size_t)a * U + (w - 1)] = rss ? access_value(T.data(), plane, L, U, a, w) : access_value_no_rss(L, a, w);
      if (!terms) continue;
      for (int term = 0; term < ACC_TERMS; ++term) {
        const int x = (term == ACC_L || term == ACC_M) ? a + w : a;
        terms[((size_t)ACC_TERMS * a + term) * U + (w - 1)] = (rss && x <= L) ? T[term * plane + (size_t)x * U + (w - 1)] : 0.;
      }
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

void access_log(Emu& E, const double* x, const uint8_t* seq, int L, const uint8_t* qual, int U, double* access, double* terms) {
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
  access_all(AccLog(ZL), m, q, in.v, out.v, ZL > NEG && ZL < HUGE_VAL, !(E.flags & F_NO_RSS), U, access, terms);
}

// 0: done in the scaled-linear form; 1: Z left the double range (or is 0), nothing written
int access_lin(Emu& E, const double* x, const uint8_t* seq, int L, const uint8_t* qual, int U, double* access, double* terms) {
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
  const double* terms5[5] = {P.e_stack.data(), P.e_ext.data(), P.e_ml.data(), P.e_close.data(), P.e_hp.data()};
  for (int k = 0; k < 2; ++k) {
    for (int t = 0; t < 5; ++t)
      for (size_t c = 0; c < nc; ++c) xwc[(size_t)(k * 5 + t) * nc + c] = lin_weight(m.lambda[k], terms5[t][c]);
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
  access_all(AccLin(1. / Z), m, q, in.v, out.v, true, !(E.flags & F_NO_RSS), U, access, terms);
  return 0;
}

}  // namespace

extern "C" {

// access: U * L doubles, access[U * p + (w - 1)]; terms: NULL or 4 * U * L doubles, the four terms of every window
// (terms[(4 * p + term) * U + (w - 1)], term 0 = T_L, 1 = T_O, 2 = T_2, 3 = T_M).  form 0: the scaled-linear form, and the log-space
// form where Z leaves the double range or the sequence has no parse (as the engine hands such a sequence on); form 1: the
// log-space form.  Returns the form that wrote the result, or -1 with emu_last_error.
int emu_access_seq(void* h, const double* x, const uint8_t* seq, int L, const uint8_t* qual, int form, int U, double* access,
                   double* terms) {
  try {
    Emu& E = *(Emu*)h;
    if (U < 1 || U > kAccessMaxWidth) throw std::runtime_error("max_width must lie in 1 .. 64");
    if (form == 0 && access_lin(E, x, seq, L, qual, U, access, terms) == 0) return 0;
    access_log(E, x, seq, L, qual, U, access, terms);
    return 1;
  } catch (std::exception& e) { g_err = e.what(); return -1; }
}

}  // extern "C"
