// Test-only CPU driver of the outside L plane behind the sweep (option loop_outside): pass 0 of the reference
// schedule (terminals ari and nasi, Z = Z(ari, nasi)) of one sequence in the scaled-linear form with the table-driven unary
// phases, the way the GPU runs it with the option on -- the outside sweep in its LPOST form (fast_outside_unary<.., LPOST>, role 0
// of the item sums alone), then the rule functions of k4_out_seed and k4_out_loops (loop_outside_seed_term, loop_outside_entry;
// lin_fast.h) cell by cell over the finished tables.  Not part of the product.
// With LOOP_OUTSIDE_MAIN it is a program of its own (for a sanitizer build): argv[1] = an energy parameter file.
#include "emul/emul.cpp"

#include <cstdio>
#include <fstream>
#include <sstream>

namespace {

// one cell of the outside sweep in the LPOST form: fast_outside_cell (emul.cpp) without the roles 1 and 2 of the item sums and
// with the L part of the unary phase left out
template <class Sink>
void lpost_outside_cell(LinOutCtx<Sink>& x0, int d, int i) {
  const ModelView& m = x0.m;
  const SeqView& q = x0.q;
  const TableView& in = x0.in;
  const TableView& out = x0.out;
  const AutomatonLayout& A = m.lay;
  const int32_t* G = m.ints;
  const double* lin = m.lin;
  const int NL = A.n_lane, L = q.L, W = q.W, j = i + d, W1 = W + 1, nq = A.n_quad;
  std::vector<double> h(4 * NL, 0.);
  double* h1 = h.data();
  double* h2 = h1 + NL;
  double* hp = h2 + NL;
  const int dmi = q.dmin[i];
  for (int p = 0; p < A.n_ap; ++p) {
    const int32_t* PR = G + A.fpr_out + 8 * p;
    const int s1 = PR[1] & 0xff, cP = fcol(PR[0], 1);
    if (dmi > 0 && dmi <= d) {
      const int hi = (W - d < L - j) ? W - d : L - j;
      double acc = 0.;
      for_mask_bits(q.okbits, j * W1, 1, hi, [&](int sp) { acc = fma(out.lda(d + sp, i, p, true), in.ldc(ST_B, sp, j, cP, true), acc); });
      if (acc != 0.) h1[s1] += acc;
    }
  }
  if (q.pair_ok(i, d))
    for (int b = 1; b <= W - d; ++b) {
      const int ii = i - b;
      const int dmii = ii >= 0 ? (int)q.dmin[ii] : 0;
      if (!(dmii > 0 && b >= dmii)) continue;
      for (int p = 0; p < A.n_ap; ++p) {
        const int32_t* PR = G + A.fpr_out + 8 * p;
        const double term = out.lda(d + b, ii, p, true) * in.ldc(ST_1, b, ii, fcol(PR[0], 0), true);
        if (term != 0.) h2[(PR[1] >> 8) & 0xff] += term;
      }
    }
  if (q.pair_ok(i, d)) {   // role 0 of the item sums
    const int cell = q.cell(i, d);
    for (int n = q.by_inner_off[cell]; n < q.by_inner_off[cell + 1]; ++n) {
      const LoopItem it = q.items[q.by_inner_idx[n]];
      const uint32_t rE = out.cidx(ST_E, it.j - it.i, it.i, 0), r1 = in.cidx(ST_L, i - it.i, it.i, 0), r2 = in.cidx(ST_L, it.j - j, j, 0);
      const uint32_t rA = in.cidx(ST_P, d, i, 0);
      const double xw0 = lin_weight(m.lambda[0], it.tsc), xw1 = lin_weight(m.lambda[1], it.tsc);
      for (int t = 0; t < nq; ++t) {
        const int qa = G[A.fqc_out + 2 * t], qb = G[A.fqc_out + 2 * t + 1];
        if (qb & (4 << 16)) continue;
        const double a0 = out.band[rE + (qa & 0xff)], a1 = in.band[r1 + ((qa >> 8) & 0xff)], a2 = in.band[r2 + ((qa >> 16) & 0xff)];
        const double aux = in.band[rA + ((qa >> 24) & 0xff)];
        const double term = a0 * (a1 * a2) * ((qb & (1 << 16)) ? xw1 : xw0);
        if (aux == 0. || term == 0.) continue;
        hp[qb & 0xffff] += term;
        x0.sink.eh((!m.lam_same && (qb & (1 << 16))) ? 1 : 0, it.tsc * term * (aux * x0.invZ));
      }
    }
  }
  double crec[kCellOutD];
  for (int k = 0; k < 12; ++k) {
    const bool on = k < 4 ? q.e_ok(i, d) : k < 6 ? q.pair_ok(i, d) : k < 8 ? (q.pair_ok(i - 1, d + 2) && q.pair_ok(i, d)) : true;
    crec[2 + k] = on ? cell_out_fetch(q, d, i, k) : 0.;
  }
  crec[0] = q.ews[i > 0 ? i - 1 : 0];
  crec[1] = q.ews[j < L ? j : L];
  const int fl = cell_out_flags(m, q, d, i);
  std::vector<double> oB(NL, 0.);
  for (int l = 0; l < NL; ++l) {
    const int s = G[A.f_live_out + l];
    oB[l] = fast_outside_unary<kFastR, kFastP, kFastL, OUT_TRAIN, true>(A, G + A.fp_out + s * kFastW, G, lin, in, out, crec, fl, d, i, x0.invZ,
                                                                         m.lam_same != 0, m.no_prf != 0, x0.sink, h1 + l, NL, 1, 0, G + A.fs_out);
  }
  for (int p = 0; p < A.n_ap; ++p) {
    const int32_t* PR = G + A.fpr_out + 8 * p;
    const int r0 = PR[0], r1 = PR[1];
    const int tg = (r0 >> 16) & 0xff;
    if (!(dmi > 0 && dmi < d)) continue;
    const bool step = d + 1 <= W && j < L && q.unp[j];
    const int nr = step ? (r1 >> 20) & 15 : 0;
    const double a_in = in.a(d, i, p);
    double acc = 0.;
    if (a_in != 0.) {
      acc = tg != 0xff ? oB[tg] : 0.;
      const double inz = a_in * x0.invZ;
      const int bj = step ? (int)q.seq[j] : 0;
      const double ewj = step ? q.ews[j] : 1.;
      for (int u = 0; u < nr; ++u) {
        const int ce = PR[5 + u], id = (ce >> 8) & 0x7fff;
        const double term = out.lda(d + 1, i, ce & 0xff, true) * (lin[A.lin_wr + 5 * id + bj] * ((G[A.fe_r + 2 * id + 1] & 1) ? ewj : 1.));
        const double z = term * inz;
        if (!m.no_prf && z != 0. && bj) x0.sink.en(G[A.fe_r + 2 * id] + bj, z);
        acc += term;
      }
    }
    out.a(d, i, p) = acc;
  }
}

// the seeds of cell (i, d): HL per lane of the unary phase, from the role-1 and role-2 records of the cell (k4_out_seed)
void seed_cell(const ModelView& m, const SeqView& q, const TableView& in, const TableView& out, int d, int i, double* hl) {
  const AutomatonLayout& A = m.lay;
  const int32_t* G = m.ints;
  const int nq = A.n_quad, cell = q.cell(i, d);
  for (int l = 0; l < A.n_lane; ++l) hl[l] = 0.;
  if (d == 0 || !(q.ubits(i, d) & UB_L)) return;
  for (int role = 1; role <= 2; ++role) {
    const int32_t* off = role == 1 ? q.by_left_off : q.by_right_off;
    const int32_t* idx = role == 1 ? q.by_left_idx : q.by_right_idx;
    const int qc0 = A.fqc_out + role * 2 * nq;
    for (int n = off[cell]; n < off[cell + 1]; ++n) {
      const LoopItem it = q.items[idx[n]];
      const uint32_t rE = out.cidx(ST_E, it.j - it.i, it.i, 0), rP = in.cidx(ST_P, it.l - it.k, it.k, 0);
      const uint32_t rL = role == 1 ? in.cidx(ST_L, it.j - it.l, it.l, 0) : in.cidx(ST_L, it.k - it.i, it.i, 0);
      const double xw0 = lin_weight(m.lambda[0], it.tsc), xw1 = lin_weight(m.lambda[1], it.tsc);
      for (int t = 0; t < nq; ++t) {
        const int qa = G[qc0 + 2 * t], qb = G[qc0 + 2 * t + 1];
        if (qb & (4 << 16)) continue;
        const double term = loop_outside_seed_term(out.band[rE + (qa & 0xff)], in.band[rP + ((qa >> 8) & 0xff)], in.band[rL + ((qa >> 16) & 0xff)],
                                                   (qb & (1 << 16)) ? xw1 : xw0);
        if (term != 0.) hl[qb & 0xffff] += term;
      }
    }
  }
}

// ENo [n_theta], EHo [2]: the statistics of the pass; outL [(L+1)][(W+1)][S]: log of the outside L plane, in the reference's
// state order and scaling, as emu_train_seq_lin exports it.  Returns 0, or 2 where Z leaves the double range.
int loop_outside_seq(Emu& E, const double* x, const uint8_t* seq, int L, const uint8_t* qual, double* ENo, double* EHo, double* outL) {
  const int nt = E.au->n_theta();
  std::vector<double> theta(x, x + nt);
  const bool no_prf = E.flags & F_NO_PRF;
  const AutomatonLayout& LY = E.lay;
  if (!LY.fp_ok) throw std::runtime_error("loop_outside: the automaton's lists do not fit the programs");
  std::vector<double> lin;
  make_lin_params(LY, E.ints.data(), theta.data(), E.tau, no_prf, &lin);
  ModelView m = make_view(LY, E.ints, theta.data(), x[nt], x[nt + 1], std::log(E.tau), no_prf, E.flags & F_NO_TURN);
  m.lin = lin.data();
  HostPlan P;
  prepare(E, P, seq, L, qual, nullptr);
  SeqView q = P.view();
  const int S = m.lay.S, W = P.W;
  const size_t nc = (size_t)(L + 1) * (W + 1), ni = P.items.size();
  std::vector<double> ews(L + 1), xwc(10 * nc), xwi(2 * ni + 1);
  for (int p = 0; p <= L; ++p) ews[p] = std::exp(P.ws[p]);
  const double* terms[5] = {P.e_stack.data(), P.e_ext.data(), P.e_ml.data(), P.e_close.data(), P.e_hp.data()};
  for (int k = 0; k < 2; ++k) {
    for (int t = 0; t < 5; ++t)
      for (size_t c = 0; c < nc; ++c) xwc[(size_t)(k * 5 + t) * nc + c] = lin_weight(m.lambda[k], terms[t][c]);
    for (size_t n = 0; n < ni; ++n) xwi[(size_t)k * ni + n] = lin_weight(m.lambda[k], P.items[n].tsc);
  }
  q.ews = ews.data(); q.xwc = xwc.data(); q.xwc_stride = nc; q.xwi = xwi.data(); q.xwi_stride = ni;
  std::vector<double> cum(L + 1, 0.);
  for (int p = 0; p < L; ++p) cum[p + 1] = cum[p] + lin[kLinPl2 + seq[p]];
  const double ln2 = 0.69314718055994530942;
  LinTab in(L, W, m.lay, E.ints.data()), out(L, W, m.lay, E.ints.data());   // (NaN-filled: a dead read shows up)
  const Constraint c0{-1, -1, 0};
  for (int d = 0; d <= W; ++d)
    for (int i = 0; i + d <= L; ++i) fast_inside_cell<false>(m, q, in.v, d, i, c0);
  for (int s = 0; s < S; ++s) in.v.o(0, s) = (s == m.lay.s00) ? 1. : 0.;
  for (int j = 1; j <= L; ++j)
    for (int s = 0; s < S; ++s) lin_inside_ext_target(m, q, in.v, j, s);
  const double Zo = lin_part(m, in.v, true, true);
  if (!(Zo > 0.) || !std::isfinite(Zo)) return 2;
  std::vector<double> en(nt + 1, 0.);
  double eh[2] = {0, 0};
  CpuSink sink{en.data(), eh, {nullptr, nullptr, nullptr}};
  LinOutCtx<CpuSink> xo{m, q, in.v, out.v, 1. / Zo, sink};
  for (int s = 0; s < S; ++s) out.v.o(L, s) = 0.;
  out.v.o(L, m.lay.s00) = 1.; out.v.o(L, m.lay.s0m1) = 1.; out.v.o(L, m.lay.s0m2) = 1.;
  for (int i = L - 1; i >= 0; --i)
    for (int s = 0; s < m.lay.n_active; ++s) lin_outside_ext_target<OUT_TRAIN>(xo, i, s);
  fast_rule7(m, q, in.v, out.v);
  for (int d = W; d >= 0; --d)
    for (int i = 0; i + d <= L; ++i) lpost_outside_cell(xo, d, i);
  // behind the sweep: the seeds into the cells' L rows (every entry), then the chain down every row
  const AutomatonLayout& A = m.lay;
  const int32_t* G = m.ints;
  const int rs = out.v.rs[ST_L], NL = A.n_lane;
  std::vector<double> hl(NL);
  for (int d = 0; d <= W; ++d)
    for (int i = 0; i + d <= L; ++i) {
      seed_cell(m, q, in.v, out.v, d, i, hl.data());
      for (int c = 0; c < rs; ++c) out.v.band[out.v.cidx(ST_L, d, i, c)] = 0.;
      for (int l = 0; l < NL; ++l) {
        const int c = fcol(G[A.fp_out + G[A.f_live_out + l] * kFastW + 2], 2);
        if (c >= 0) out.v.band[out.v.cidx(ST_L, d, i, c)] = hl[l];
      }
    }
  std::vector<double> parent(rs), row(rs);
  for (int i = 0; i <= L; ++i) {
    std::fill(parent.begin(), parent.end(), 0.);
    for (int d = (W < L - i) ? W : L - i; d >= 0; --d) {
      const int j = i + d;
      const bool eok = q.e_ok(i, d), doL = j < L && d + 1 <= W;
      const int c_up = eok ? q.cell(i - 1, d + 2) : q.cell(i, d);
      std::fill(row.begin(), row.end(), 0.);
      for (int l = 0; l < NL; ++l) {
        const int32_t* Pg = G + A.fp_out + G[A.f_live_out + l] * kFastW;
        const int c = fcol(Pg[2], 2), cEo = fcol(Pg[1], 1), kl = (Pg[0] >> 2) & 1;
        if (c < 0 || !(Pg[0] & 1) || !(q.ubits(i, d) & UB_L)) continue;
        const double inL = in.v.band[in.v.cidx(ST_L, d, i, c)];
        const double oE = (eok && cEo >= 0) ? out.v.band[out.v.cidx(ST_E, d, i, cEo)] : 0.;
        row[c] = loop_outside_entry<kFastR>(Pg, G, A.fe_r, lin.data() + A.lin_wr, parent.data(), inL, out.v.band[out.v.cidx(ST_L, d, i, c)], oE,
                                            eok ? xw_cell(q, kl, XT_HP, c_up) : 0., q.e_hp[c_up], doL, j < L ? (int)q.seq[j] : 0,
                                            q.ews[j < L ? j : L], 1. / Zo, m.lam_same ? 0 : kl, m.no_prf != 0, sink);
      }
      for (int c = 0; c < rs; ++c) out.v.band[out.v.cidx(ST_L, d, i, c)] = row[c];   // (the driver keeps the plane for the export)
      parent = row;
    }
  }
  std::copy(en.begin(), en.begin() + nt, ENo);
  EHo[0] = eh[0]; EHo[1] = eh[1];
  for (int i = 0; i <= L; ++i)
    for (int d = 0; d <= W; ++d)
      for (int s = 0; s < S; ++s) {
        double v = NEG;
        if (i + d <= L) {
          const double lv = lin_get(m, q, out.v, ST_L, d, i, s);
          v = lv > 0. ? std::log(lv) - (cum[L] - (cum[i + d] - cum[i])) * ln2 : NEG;
        }
        outL[((size_t)i * (W + 1) + d) * S + E.ints[E.lay.st_ref + s]] = v;
      }
  return 0;
}

}  // namespace

extern "C" {

int emu_loop_outside_seq(void* h, const double* x, const uint8_t* seq, int L, const uint8_t* qual, double* ENo, double* EHo, double* outL) {
  try {
    return loop_outside_seq(*(Emu*)h, x, seq, L, qual, ENo, EHo, outL);
  } catch (std::exception& e) { g_err = e.what(); return -1; }
}

}  // extern "C"

#ifdef LOOP_OUTSIDE_MAIN
int main(int argc, char** argv) {
  if (argc < 2) { fprintf(stderr, "usage: %s ENERGY_PARAMETER_FILE\n", argv[0]); return 2; }
  std::ifstream f(argv[1]);
  std::stringstream par;
  par << f.rdbuf();
  void* h = emu_create("((.*.))", par.str().c_str(), 50, 30, 1e-4, 0.1, 0);
  if (!h) { fprintf(stderr, "%s\n", emu_last_error()); return 1; }
  emu_set_prune(h, 1);   // (the lists of the pruned automaton fit the programs)
  if (!(emu_set_fast(h, 1) & 1)) { fprintf(stderr, "the automaton's lists do not fit the programs\n"); return 1; }
  const int np = emu_n_param(h), S = emu_n_state(h);
  std::vector<double> x(np, 0.);
  for (int k = 0; k < np - 2; ++k) x[k] = -1.4 + 0.6 * k / (np - 2);
  x[np - 2] = 1.0; x[np - 1] = 0.7;
  const int lens[3] = {7, 37, 60};
  for (int L : lens) {
    std::vector<uint8_t> seq(L), qual(L + 1, 10);
    unsigned r = 12345u + L;
    for (int p = 0; p < L; ++p) { r = r * 1664525u + 1013904223u; seq[p] = 1 + ((r >> 24) & 3); }
    if (L >= 7) { seq[0] = 3; seq[1] = 2; seq[L - 2] = 3; seq[L - 1] = 2; }   // (G C ... G C: a pair at either end)
    qual[L] = 0;
    const int W = L < 50 ? L : 50;
    std::vector<double> en(np), eh(2), outL((size_t)(L + 1) * (W + 1) * S);
    const int rc = emu_loop_outside_seq(h, x.data(), seq.data(), L, qual.data(), en.data(), eh.data(), outL.data());
    if (rc < 0) { fprintf(stderr, "%s\n", emu_last_error()); return 1; }
    double sum = 0.;
    for (int k = 0; k < np - 2; ++k) sum += en[k];
    printf("L %d rc %d sum EN %.12g EH %.12g %.12g\n", L, rc, sum, eh[0], eh[1]);
  }
  emu_destroy(h);
  return 0;
}
#endif
