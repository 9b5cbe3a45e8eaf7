// ctx_kernels.hip -- structural context profiles under the motif model (rule in ctx_rules.h).  k_ctx_cells runs on
// the compact tables of the scan's first sum pass (launch_lin_scan_group, SCAN_PASS_START), right behind it on the same slots and
// stream, before the next group of the stream reuses them: one lane per run [i, i + d) for its u, h and b, and one lane per
// position for the exterior column (the pair posteriors P(i, d) of the same slots come from k4_pairs).  k_ctx_seq, one workgroup
// per sequence, turns the per-run values into the seven columns; it serves the log-space form too, whose per-run values the
// fused scan kernel writes (DpArgs::ctx).  No atomics: every sum has a fixed order, so repeats over the same tables give the same
// bits.  A sequence the range check flagged is left to the log-space form.
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "lin_views.h"
#include "ctx_rules.h"

namespace elemdp {

// one lane per cell (i fastest: neighbouring lanes take neighbouring runs of a diagonal and read neighbouring rows);
// grid (cells / kThreads, G).  The bulge terms walk the run's by-left and by-right item lists of the plan once and form an item's
// weight exp(lambda_k tsc) from its record: LinArgs::xwi is null for a scan (the band kernels form the weights where they stage
// the records), so there is no per-item weight array to read.
__global__ __launch_bounds__(kThreads) void k_ctx_cells(LinArgs a, CtxArgs c) {
  __shared__ AutomatonLayout s_lay;
  {
    const int32_t* src = reinterpret_cast<const int32_t*>(a.layp);
    int32_t* dst = reinterpret_cast<int32_t*>(&s_lay);
    for (int t = threadIdx.x; t < (int)(sizeof(AutomatonLayout) / sizeof(int32_t)); t += kThreads) dst[t] = src[t];
  }
  __syncthreads();
  const int g = blockIdx.y;
  LViews v(s_lay);
  make_lviews(a, g, v);
  if (v.row[4] != 0.) return;   // (outside the double range: the log-space form of the fused scan kernel covers it)
  const int L = v.q.L, W = v.q.W;
  const int t = blockIdx.x * kThreads + threadIdx.x;
  if (t >= (L + 1) * (W + 1)) return;
  const CtxLin f{1. / v.zs[0]};
  if (t < L) c.o[(size_t)g * c.o_stride + t] = ctx_exterior(f, v.m, v.q, v.in, v.out, t);
  const int d = t / (L + 1), i = t - d * (L + 1);
  CtxCell r{0., 0., 0.};
  if (d >= 1 && i + d <= L) r = ctx_cell(f, v.m, v.q, v.in, v.out, d, i);
  const size_t at = (size_t)g * c.c_stride + (size_t)i * (W + 1) + d;
  c.u[at] = r.u;
  c.h[at] = r.h;
  c.b[at] = r.b;
}

// one workgroup per sequence: the difference arrays of h and b, their prefix sums over the positions in tiles of kThreads (a
// fixed tree per tile in LDS, the carry from tile to tile), the sums of P and u per position, the remainders; 7 L doubles
__global__ __launch_bounds__(kThreads) void k_ctx_seq(CtxArgs c) {
  __shared__ double s_h[kThreads], s_b[kThreads];
  const int g = blockIdx.x, tid = threadIdx.x;
  const int n = c.idx[g];
  if (c.skip_flagged && c.seq_out[(size_t)n * c.out_stride + 4] != 0.) return;
  const SeqPlan p = c.plans[n];
  const int L = p.L, W = p.W;
  double* prof = c.profile + (size_t)CTX_COLS * p.seq_base;
  if (c.no_rss) {
    for (int q = tid; q < L; q += kThreads) ctx_row_exterior(prof + (size_t)CTX_COLS * q);
    return;
  }
  const double* P = c.P + (size_t)g * c.c_stride;
  const double* U = c.u + (size_t)g * c.c_stride;
  const double* H = c.h + (size_t)g * c.c_stride;
  const double* B = c.b + (size_t)g * c.c_stride;
  const double* O = c.o + (size_t)g * c.o_stride;
  double carry_h = 0., carry_b = 0.;
  for (int t0 = 0; t0 < L; t0 += kThreads) {
    const int q = t0 + tid;
    const bool live = q < L;
    s_h[tid] = live ? ctx_diff(H, L, W, q) : 0.;
    s_b[tid] = live ? ctx_diff(B, L, W, q) : 0.;
    __syncthreads();
    for (int off = 1; off < kThreads; off <<= 1) {
      const double uh = tid >= off ? s_h[tid - off] : 0., ub = tid >= off ? s_b[tid - off] : 0.;
      __syncthreads();
      s_h[tid] += uh;
      s_b[tid] += ub;
      __syncthreads();
    }
    if (live)
      ctx_compose(O[q], ctx_sum_from(P, L, W, q), ctx_sum_to(P, L, W, q + 1), ctx_sum_to(U, L, W, q + 1), carry_h + s_h[tid],
                  carry_b + s_b[tid], prof + (size_t)CTX_COLS * q);
    carry_h += s_h[kThreads - 1];
    carry_b += s_b[kThreads - 1];
    __syncthreads();
  }
}

hipError_t launch_ctx_cells(const LinArgs& a, const CtxArgs& c, int G, int cells_max, hipStream_t st) {
  if (G <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_ctx_cells, dim3((cells_max + kThreads - 1) / kThreads, G), dim3(kThreads), 0, st, lin_in_world(a), c);
  return hipGetLastError();
}
hipError_t launch_ctx_seq(const CtxArgs& c, int G, hipStream_t st) {
  if (G <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_ctx_seq, dim3(G), dim3(kThreads), 0, st, c);
  return hipGetLastError();
}

}  // namespace elemdp
