// Test-only CPU driver of the sampler in one world: the inside tables of the scan's first sum pass on the CPU, as
// tests/sample_emul.cpp builds them, then the walk of sample_rules.h with the world's terminals alone.  Not part of the product.
#include "emul/emul.cpp"

#include "../rnaelem_amd/csrc/sample_rules.h"

extern "C" {

// n_samples derivations of one sequence in world 0 (mixture), 1 (motif) or 2 (none): rss / node n_samples x L bytes, logp
// n_samples values; a failed walk leaves its sample blank with node 0 and a NaN log-probability, as sample_one does on the device.
// Returns the SampleStatus, or -1 with emu_last_error on a failure of the driver itself
int emu_world_sample_seq_lin(void* h, const double* x, const uint8_t* seq, int L, const uint8_t* qual, int n_samples, uint64_t seed,
                             uint64_t index, char* rss, uint8_t* node, double* logp, int world) {
  try {
    Emu& E = *(Emu*)h;
    const int nt = E.au->n_theta();
    std::vector<double> theta(x, x + nt);
    if (E.flags & F_SOFTMAX)
      for (int r = 0; r < E.au->n_rows(); ++r) {
        double tot = NEG;
        for (int c = 0; c < E.au->row_width(r); ++c) tot = lse2(tot, x[E.au->row_offset(r) + c]);
        for (int c = 0; c < E.au->row_width(r); ++c) theta[E.au->row_offset(r) + c] = x[E.au->row_offset(r) + c] - tot;
      }
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
    LinTab in(L, P.W, m.lay, E.ints.data());   // (NaN-filled: a dead read of the walk shows up)
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
    const LinSampleTab T{in.v};
    const int cap = elemdp::sample_stack_cap(L);
    std::vector<TraceFrame> stack(cap + 3);   // (a step pushes up to three frames past a bound it has checked)
    int status = SAMPLE_OK;
    for (int k = 0; k < n_samples; ++k) {
      char* r = rss + (size_t)k * L;
      uint8_t* nd = node + (size_t)k * L;
      std::fill(r, r + L, ' ');
      std::fill(nd, nd + L, (uint8_t)0);
      double lp = std::numeric_limits<double>::quiet_NaN();
      const int st = sample_walk(m, q, T, seed, index, (uint64_t)k, nd, r, &lp, stack.data(), cap, world);
      if (st != SAMPLE_OK) {
        lp = std::numeric_limits<double>::quiet_NaN();
        std::fill(r, r + L, ' ');
        std::fill(nd, nd + L, (uint8_t)0);
      }
      logp[k] = lp;
      status = std::max(status, st);
    }
    return status;
  } catch (std::exception& e) { g_err = e.what(); return -1; }
}

}  // extern "C"
