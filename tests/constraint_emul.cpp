// Test-only CPU driver of the hard structure constraints: prepare() as elemdp_load_batch does it, then the host rule of
// constraint_rules.h on the plan's pair mask, its unp and ndot rows (what k_constrain and Engine::constrain do on the device),
// plan_finish() with the structure imposed, and the product's rules of the scan's first sum pass on the CPU -- scaled-linear on
// compact tables (plain and table-driven unary phases) and log space on dense ones --, then ln Z, the pair posteriors (the P plane
// of pair_rules.h's definition: inside times outside over Z), the unpaired row and the context profile of ctx_rules.h on the
// finished tables.  Not part of the product.
#include "emul/emul.cpp"

#include "../rnaelem_amd/csrc/constraint_rules.h"
#include "../rnaelem_amd/csrc/ctx_rules.h"

namespace {

// the constrained plan of one sequence; throws what the load would refuse
void prepare_constrained(const Emu& E, HostPlan& P, const uint8_t* seq, int L, const uint8_t* qual, const char* cons) {
  prepare(E, P, seq, L, qual, nullptr);
  std::vector<uint8_t> cls(L);
  std::vector<int32_t> partner(L), enc(L);
  P.ndot.assign(L + 1, 0);
  const int min_span = (E.flags & F_NO_TURN) ? 1 : 5;
  const auto pair_ok = [&](int i, int j) { return canonical_pair(P.seq.data(), L, P.W, min_span, i, j - i + 1); };
  const std::string err = constraint_derive(cons, L, 0, pair_ok, cls.data(), partner.data(), enc.data(), P.unp.data(), P.ndot.data());
  if (!err.empty()) throw std::runtime_error(err);
  const ConsView c{cls.data(), partner.data(), enc.data()};
  for (size_t w = 0; w < P.okbits.size(); ++w) P.okbits[w] = cons_word(c, L, P.W, (int)w, P.okbits[w]);
  P.have_fix = true;
  plan_finish(E, P);
}

// P(i, d) and the unpaired row from the finished tables
template <class F>
void pair_rows(const F& f, const ModelView& m, const SeqView& q, const TableView& in, const TableView& out, bool parse, double* Pout, double* unp) {
  const int L = q.L, W = q.W;
  for (size_t c = 0; c < (size_t)(L + 1) * (W + 1); ++c) Pout[c] = 0.;
  for (int p = 0; p < L; ++p) unp[p] = 1.;
  if (!parse) return;
  for (int i = 0; i <= L; ++i)
    for (int d = 1; d <= W && i + d <= L; ++d) {
      if (!q.pair_ok(i, d)) continue;
      double acc = 0.;
      for (int s = 0; s < m.lay.S; ++s)
        if (s != m.lay.shadow) acc += f.post(f.mul(f.ld(in, ST_P, d, i, s), f.ld(out, ST_P, d, i, s)));
      Pout[(size_t)i * (W + 1) + d] = acc;
      unp[i] -= acc; unp[i + d - 1] -= acc;
    }
}

template <class F>
void ctx_profile(const F& f, const ModelView& m, const SeqView& q, const TableView& in, const TableView& out, bool parse, double* profile) {
  const int L = q.L, W = q.W;
  if (!parse) {
    for (int p = 0; p < L; ++p) ctx_row_exterior(profile + (size_t)CTX_COLS * p);
    return;
  }
  const size_t nc = (size_t)(L + 1) * (W + 1);
  std::vector<double> P(nc, 0.), U(nc, 0.), H(nc, 0.), B(nc, 0.), O(L + 1, 0.);
  for (int i = 0; i <= L; ++i)
    for (int d = 1; d <= W && i + d <= L; ++d) {
      const size_t c = (size_t)i * (W + 1) + d;
      if (q.pair_ok(i, d)) {
        double acc = 0.;
        for (int s = 0; s < m.lay.S; ++s)
          if (s != m.lay.shadow) acc += f.post(f.mul(f.ld(in, ST_P, d, i, s), f.ld(out, ST_P, d, i, s)));
        P[c] = acc;
      }
      const CtxCell r = ctx_cell(f, m, q, in, out, d, i);
      U[c] = r.u; H[c] = r.h; B[c] = r.b;
    }
  for (int p = 0; p < L; ++p) O[p] = ctx_exterior(f, m, q, in, out, p);
  ctx_finish(P.data(), U.data(), H.data(), B.data(), O.data(), L, W, profile);
}

void softmax_theta(const Emu& E, const double* x, std::vector<double>& theta) {
  if (!(E.flags & F_SOFTMAX)) return;
  for (int r = 0; r < E.au->n_rows(); ++r) {
    double tot = NEG;
    for (int c = 0; c < E.au->row_width(r); ++c) tot = lse2(tot, x[E.au->row_offset(r) + c]);
    for (int c = 0; c < E.au->row_width(r); ++c) theta[E.au->row_offset(r) + c] = x[E.au->row_offset(r) + c] - tot;
  }
}

void ctx_log(Emu& E, const double* x, const uint8_t* seq, int L, const uint8_t* qual, const char* cons, double* lnZ, double* Pout, double* unp, double* profile) {
  const int nt = E.au->n_theta();
  std::vector<double> theta(x, x + nt);
  softmax_theta(E, x, theta);
  ModelView m = make_view(E.lay, E.ints, theta.data(), x[nt], x[nt + 1], std::log(E.tau), E.flags & F_NO_PRF, E.flags & F_NO_TURN);
  HostPlan P;
  prepare_constrained(E, P, seq, L, qual, cons);
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
  const bool parse = ZL > NEG && ZL < HUGE_VAL && !(E.flags & F_NO_RSS);
  *lnZ = ZL;
  pair_rows(CtxLog{ZL}, m, q, in.v, out.v, parse, Pout, unp);
  ctx_profile(CtxLog{ZL}, m, q, in.v, out.v, parse, profile);
}

// 0: done in the scaled-linear form; 1: Z left the double range (or is 0), nothing written
int ctx_lin(Emu& E, const double* x, const uint8_t* seq, int L, const uint8_t* qual, const char* cons, double* Pout, double* unp, double* profile) {
  const int nt = E.au->n_theta();
  std::vector<double> theta(x, x + nt);
  softmax_theta(E, x, theta);
  const bool no_prf = E.flags & F_NO_PRF;
  std::vector<double> lin;
  make_lin_params(E.lay, E.ints.data(), theta.data(), E.tau, no_prf, &lin);
  ModelView m = make_view(E.lay, E.ints, theta.data(), x[nt], x[nt + 1], std::log(E.tau), no_prf, E.flags & F_NO_TURN);
  m.lin = lin.data();
  HostPlan P;
  prepare_constrained(E, P, seq, L, qual, cons);
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
  q.xwi = nullptr; q.xwi_stride = 0;   // (as on the device: the engine keeps no per-item weights, the rule forms them itself)
  pair_rows(CtxLin{1. / Z}, m, q, in.v, out.v, true, Pout, unp);
  ctx_profile(CtxLin{1. / Z}, m, q, in.v, out.v, !(E.flags & F_NO_RSS), profile);
  return 0;
}

}  // namespace

extern "C" {

// One sequence under the constraint string cons (L characters).  lnZ: ln Z(ari, nasi) of the constrained ensemble, from the
// log-space sweep (-inf: no parse); P: (L+1) * (W+1) pair posteriors; unp: L; profile: 7 * L, columns O L R H B I M.  form 0: the
// scaled-linear form for P, unp and the profile (the log-space form where Z leaves the double range or the sequence has no
// parse); form 1: the log-space form.  Returns the form that wrote them, or -1 with emu_last_error (a refused string).
int emu_constraint_seq(void* h, const double* x, const uint8_t* seq, int L, const uint8_t* qual, const char* cons, int form,
                       double* lnZ, double* P, double* unp, double* profile) {
  try {
    Emu& E = *(Emu*)h;
    std::vector<double> P1((size_t)(L + 1) * (std::min(L, E.max_span) + 1)), u1(L), prof1((size_t)7 * L);
    ctx_log(E, x, seq, L, qual, cons, lnZ, form == 0 ? P1.data() : P, form == 0 ? u1.data() : unp, form == 0 ? prof1.data() : profile);
    if (form != 0) return 1;
    if (ctx_lin(E, x, seq, L, qual, cons, P, unp, profile) == 0) return 0;
    std::copy(P1.begin(), P1.end(), P); std::copy(u1.begin(), u1.end(), unp); std::copy(prof1.begin(), prof1.end(), profile);
    return 1;
  } catch (std::exception& e) { g_err = e.what(); return -1; }
}

}  // extern "C"
