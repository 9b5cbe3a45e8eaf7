// Test-only CPU driver of the loop posteriors: the product's rules of the scan's first sum pass on the CPU, as
// emu_scan_seq_lin (scaled-linear, compact tables) and emu_scan_seq (log space, dense tables) run them, then the rule of
// loop_rules.h on the finished tables, one lane per cell, next to the pair posterior, H(., 2) of helix_rules.h and the context
// profile of ctx_rules.h on the same tables (the identities of the tests).  Not part of the product.
#include "emul/emul.cpp"

#include "../rnaelem_amd/csrc/loop_rules.h"

namespace {

struct LoopJob {
  double min_prob;
  double* cols;      // 5 (W+1) (L+1) doubles, cols[(c (W+1) + d) (L+1) + i], columns H S B I M; 0 where the cell is no unit
  double* P;         // (W+1) (L+1) doubles, P[d (L+1) + i]: the pair posterior in the order of the product's reduction
  double* H2;        // the same shape: H(i, d, 2) of helix_rules.h
  double* profile;   // 7 L doubles: the context profile of ctx_rules.h on the same tables
  int64_t cap; int64_t* n_two; int32_t* t_i; int32_t* t_j; int32_t* t_k; int32_t* t_l; double* t_p;   // the two-loop list
  int n_loops; const int32_t* s_type; const int32_t* s_i; const int32_t* s_d; const int32_t* s_k; const int32_t* s_l; double* s_p;
};

// live false: no parse at all, or a model without secondary structure (the tables are not read)
template <class F>
void loop_all(const F& f, const ModelView& m, const SeqView& q, const TableView& in, const TableView& out, bool live, const LoopJob& job) {
  const int L = q.L, W = q.W, S = m.lay.S;
  const size_t nc = (size_t)(W + 1) * (L + 1);
  for (size_t t = 0; t < LOOP_COLS * nc; ++t) job.cols[t] = 0.;
  for (size_t t = 0; t < nc; ++t) job.P[t] = job.H2[t] = 0.;
  for (int t = 0; t < job.n_loops; ++t) job.s_p[t] = 0.;
  *job.n_two = 0;
  for (int p = 0; p < L; ++p) ctx_row_exterior(job.profile + (size_t)CTX_COLS * p);
  if (!live) return;
  std::vector<double> v0(S), v1(S), row(2), T(q.by_outer_off[(size_t)(L + 1) * (W + 1)] + 1, 0.);
  const OneLane ln;
  const double bound = loop_pick_bound(job.min_prob);
  {
    std::vector<double> Pc((size_t)(L + 1) * (W + 1), 0.), U(Pc), H(Pc), B(Pc), O(L + 1, 0.);
    for (int i = 0; i <= L; ++i)
      for (int d = 1; d <= W && i + d <= L; ++d) {
        const size_t c = (size_t)i * (W + 1) + d;
        if (q.pair_ok(i, d)) {
          double acc = 0.;
          for (int s = 0; s < S; ++s)
            if (s != m.lay.shadow) acc += f.post(f.mul(f.ld(in, ST_P, d, i, s), f.ld(out, ST_P, d, i, s)));
          Pc[c] = acc;
          job.P[(size_t)d * (L + 1) + i] = acc;
        }
        const CtxCell r = ctx_cell(f, m, q, in, out, d, i);
        U[c] = r.u; H[c] = r.h; B[c] = r.b;
      }
    for (int p = 0; p < L; ++p) O[p] = ctx_exterior(f, m, q, in, out, p);
    ctx_finish(Pc.data(), U.data(), H.data(), B.data(), O.data(), L, W, job.profile);
  }
  for (int i = 0; i <= L; ++i)
    for (int d = 2; d <= W && i + d <= L; ++d) {
      if (!q.pair_ok(i, d)) continue;
      const HelixRun r = helix_chain(f, ln, m, q, in, out, i, d, 2, 0., v0.data(), v1.data(), row.data());
      if (r.n >= 2) job.H2[(size_t)d * (L + 1) + i] = row[1];
      if (!(job.P[(size_t)d * (L + 1) + i] >= bound)) continue;
      double cols[LOOP_COLS];
      loop_cell(f, m, q, in, out, i, d, cols, T.data());
      for (int c = 0; c < LOOP_COLS; ++c) job.cols[((size_t)c * (W + 1) + d) * (L + 1) + i] = cols[c];
      const int oc = q.cell(i + 1, d - 2);
      for (int it = q.by_outer_off[oc]; it < q.by_outer_off[oc + 1]; ++it) {
        if (!loop_item_live(q, it) || !(T[it] >= job.min_prob)) continue;
        const int64_t at = (*job.n_two)++;
        if (at >= job.cap) continue;
        job.t_i[at] = i; job.t_j[at] = i + d; job.t_k[at] = q.items[it].k; job.t_l[at] = q.items[it].l; job.t_p[at] = T[it];
      }
    }
  for (int t = 0; t < job.n_loops; ++t)
    job.s_p[t] = loop_of_structure(f, m, q, in, out, job.s_type[t], job.s_i[t], job.s_d[t], job.s_k[t], job.s_l[t]);
}

void softmax_theta(const Emu& E, const double* x, std::vector<double>& theta) {
  if (!(E.flags & F_SOFTMAX)) return;
  for (int r = 0; r < E.au->n_rows(); ++r) {
    double tot = NEG;
    for (int c = 0; c < E.au->row_width(r); ++c) tot = lse2(tot, x[E.au->row_offset(r) + c]);
    for (int c = 0; c < E.au->row_width(r); ++c) theta[E.au->row_offset(r) + c] = x[E.au->row_offset(r) + c] - tot;
  }
}

void loop_log(Emu& E, const double* x, const uint8_t* seq, int L, const uint8_t* qual, const LoopJob& job) {
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
  loop_all(LoopLog(ZL), m, q, in.v, out.v, ZL > NEG && ZL < HUGE_VAL && !(E.flags & F_NO_RSS), job);
}

// 0: done in the scaled-linear form; 1: Z left the double range (or is 0), nothing written
int loop_lin(Emu& E, const double* x, const uint8_t* seq, int L, const uint8_t* qual, const LoopJob& job) {
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
  loop_all(LoopLin(1. / Z), m, q, in.v, out.v, !(E.flags & F_NO_RSS), job);
  return 0;
}

}  // namespace

extern "C" {

// the span W the plan of a sequence of length L has (the row length of the outputs)
int emu_loop_span(void* h, const uint8_t* seq, int L, const uint8_t* qual) {
  try {
    Emu& E = *(Emu*)h;
    HostPlan P;
    prepare(E, P, seq, L, qual, nullptr);
    return P.W;
  } catch (std::exception& e) { g_err = e.what(); return -1; }
}

// The loop posteriors of one sequence (LoopJob).  form 0: the scaled-linear form, and the log-space form where Z leaves the double
// range or the sequence has no parse (as the engine hands such a sequence on); form 1: the log-space form.  Returns the form that
// wrote the outputs, or -1 with emu_last_error.  *n_two may exceed cap: then only the first cap entries are written.
int emu_loop_seq(void* h, const double* x, const uint8_t* seq, int L, const uint8_t* qual, int form, double min_prob, double* cols,
                 double* P, double* H2, double* profile, int64_t cap, int64_t* n_two, int32_t* t_i, int32_t* t_j, int32_t* t_k,
                 int32_t* t_l, double* t_p, int n_loops, const int32_t* s_type, const int32_t* s_i, const int32_t* s_d,
                 const int32_t* s_k, const int32_t* s_l, double* s_p) {
  try {
    Emu& E = *(Emu*)h;
    const LoopJob job{min_prob, cols, P, H2, profile, cap, n_two, t_i, t_j, t_k, t_l, t_p, n_loops, s_type, s_i, s_d, s_k, s_l, s_p};
    if (form == 0 && loop_lin(E, x, seq, L, qual, job) == 0) return 0;
    loop_log(E, x, seq, L, qual, job);
    return 1;
  } catch (std::exception& e) { g_err = e.what(); return -1; }
}

}  // extern "C"
