// Test-only CPU driver of the pair posteriors by motif node pair: the product's rules of the scan's first sum pass
// on the CPU, as emu_scan_seq_lin (scaled-linear, compact tables) and emu_scan_seq (log space, dense tables) run them, then the
// rule of stem_rules.h on the finished tables, over the lists the engine builds (stem_lists_build).  Not part of the product.
// With STEM_EMUL_MAIN it is a stand-alone program (for a sanitiser run): stem_emul PARAM_FILE.
#include "emul/emul.cpp"

#include "../rnaelem_amd/csrc/stem_rules.h"

namespace {

// live false: no parse at all, or a model without secondary structure (the tables are not read).  Q: (L+1)(W+1) K doubles in the
// layout of stem_at; counts: 25 K doubles.
template <class F>
void stem_profile(const F& f, const Emu& E, const ModelView& m, const SeqView& q, const TableView& in, const TableView& out, bool live,
                  int parts, double* Q, double* counts) {
  const int L = q.L, W = q.W;
  std::vector<int32_t> blob;
  const int K = stem_lists_build(m.lay, E.ints.data(), &blob);
  const StemLists sl{blob.data(), K, parts};
  for (int k = 0; k < K; ++k)
    for (int d = 0; d <= W; ++d)
      for (int i = 0; i + d <= L; ++i) Q[stem_at(L, W, k, i, d)] = live ? stem_value(f, sl, m, q, in, out, d, i, k) : 0.;
  for (int t = 0; t < K * kStemBlock; ++t) counts[t] = live ? stem_count(Q, q.seq, q.okbits, L, W, t) : 0.;
}

void softmax_theta(const Emu& E, const double* x, std::vector<double>& theta) {
  if (!(E.flags & F_SOFTMAX)) return;
  for (int r = 0; r < E.au->n_rows(); ++r) {
    double tot = NEG;
    for (int c = 0; c < E.au->row_width(r); ++c) tot = lse2(tot, x[E.au->row_offset(r) + c]);
    for (int c = 0; c < E.au->row_width(r); ++c) theta[E.au->row_offset(r) + c] = x[E.au->row_offset(r) + c] - tot;
  }
}

void stem_log(Emu& E, const double* x, const uint8_t* seq, int L, const uint8_t* qual, int parts, double* Q, double* counts) {
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
  stem_profile(StemLog{ZL}, E, m, q, in.v, out.v, ZL > NEG && ZL < HUGE_VAL && !(E.flags & F_NO_RSS), parts, Q, counts);
}

// 0: done in the scaled-linear form; 1: Z left the double range (or is 0), nothing written
int stem_lin(Emu& E, const double* x, const uint8_t* seq, int L, const uint8_t* qual, int parts, double* Q, double* counts) {
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
  stem_profile(StemLin{1. / Z}, E, m, q, in.v, out.v, !(E.flags & F_NO_RSS), parts, Q, counts);
  return 0;
}

}  // namespace

extern "C" {

// the stem slots of the handle's automaton: writes up to cap node pairs, returns K
int emu_stem_slots(void* h, int32_t* node_left, int32_t* node_right, int cap) {
  Emu& E = *(Emu*)h;
  std::vector<int32_t> blob;
  const int K = stem_lists_build(E.lay, E.ints.data(), &blob);
  for (int k = 0; k < K && k < cap; ++k) { node_left[k] = blob[K + 1 + 2 * k]; node_right[k] = blob[K + 2 + 2 * k]; }
  return K;
}

// the span W the plan of a sequence of length L has (the row length of Q)
int emu_stem_span(void* h, const uint8_t* seq, int L, const uint8_t* qual) {
  try {
    Emu& E = *(Emu*)h;
    HostPlan P;
    prepare(E, P, seq, L, qual, nullptr);
    return P.W;
  } catch (std::exception& e) { g_err = e.what(); return -1; }
}

// Q: (L+1)(W+1) K doubles, Q[(k (W+1) + d) (L+1) + i] (entries with i + d > L are not written); counts: 25 K doubles.  form 0: the
// scaled-linear form, and the log-space form where Z leaves the double range or the sequence has no parse (as the engine hands
// such a sequence on); form 1: the log-space form.  parts: StemPart bits (3 = the product).  Returns the form that wrote Q, or
// -1 with emu_last_error.
int emu_stem_seq(void* h, const double* x, const uint8_t* seq, int L, const uint8_t* qual, int form, int parts, double* Q, double* counts) {
  try {
    Emu& E = *(Emu*)h;
    if (form == 0 && stem_lin(E, x, seq, L, qual, parts, Q, counts) == 0) return 0;
    stem_log(E, x, seq, L, qual, parts, Q, counts);
    return 1;
  } catch (std::exception& e) { g_err = e.what(); return -1; }
}

}  // extern "C"

#ifdef STEM_EMUL_MAIN
#include <cstdio>
#include <fstream>
#include <sstream>

// both forms and both unary forms at L = 47 .. 107 and W = 20 .. 70; prints the largest difference between the two forms and the
// largest |sum of the counts - sum of Q|
int main(int argc, char** argv) {
  if (argc < 2) { std::fprintf(stderr, "usage: stem_emul PARAM_FILE\n"); return 2; }
  std::ifstream fin(argv[1]);
  std::stringstream ss;
  ss << fin.rdbuf();
  const std::string par = ss.str();
  double worst = 0., worst_c = 0., mass = 0.;
  const int shapes[4][2] = {{47, 20}, {60, 35}, {107, 20}, {107, 70}};
  for (const auto& sh : shapes) {
    const int L = sh[0], W = sh[1];
    void* h = emu_create("((.*.))", par.c_str(), W, 30, 1e-4, 0.1, 0);
    if (!h) { std::fprintf(stderr, "%s\n", emu_last_error()); return 1; }
    Emu& E = *(Emu*)h;
    const int np = E.au->n_theta() + 2;
    std::vector<double> x(np);
    for (int k = 0; k < np - 2; ++k) x[k] = -1.4 + 0.6 * ((k * 7) % 11) / 11.;
    x[np - 2] = 1.0; x[np - 1] = 0.7;
    std::vector<uint8_t> seq(L), qual(L + 1, 10);
    uint32_t r = 12345u + L;
    for (int p = 0; p < L; ++p) { r = r * 1664525u + 1013904223u; seq[p] = 1 + ((r >> 24) & 3); }
    const int Ws = emu_stem_span(h, seq.data(), L, qual.data());
    const int K = emu_stem_slots(h, nullptr, nullptr, 0);
    const size_t nq = (size_t)(L + 1) * (Ws + 1) * K;
    std::vector<double> first;
    for (int fast = 0; fast < 2; ++fast) {
      emu_set_fast(h, fast);
      for (int form = 0; form < 2; ++form) {
        std::vector<double> Q(nq, 0.), counts((size_t)K * kStemBlock);
        if (emu_stem_seq(h, x.data(), seq.data(), L, qual.data(), form, SP_ALL, Q.data(), counts.data()) < 0) {
          std::fprintf(stderr, "%s\n", emu_last_error());
          return 1;
        }
        double sq = 0., sc = 0.;
        for (double v : Q) sq += v;
        for (double v : counts) sc += v;
        worst_c = std::max(worst_c, std::fabs(sq - sc));
        mass = std::max(mass, sq);
        if (first.empty()) first = Q;
        for (size_t t = 0; t < nq; ++t) worst = std::max(worst, std::fabs(Q[t] - first[t]));
      }
    }
    emu_destroy(h);
  }
  std::printf("pairs %.3f, forms differ by %.3g, counts differ from Q by %.3g\n", mass, worst, worst_c);
  return worst < 1e-9 && worst_c < 1e-9 && mass > 1. ? 0 : 1;
}
#endif
