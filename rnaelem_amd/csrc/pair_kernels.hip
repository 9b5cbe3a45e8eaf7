// pair_kernels.hip -- base-pair posteriors under the motif model: the reduction over the compact tables of the
// scan's first sum pass (k4_pairs), the per-sequence unpaired sums and compaction (k_pair_seq), and the batch list in
// (sequence, i, j) order (k_pair_kept, k_pair_prefix, k_list_scatter; the conditional and the stem call build their lists with the
// same three).  No atomics: every sum has a fixed order, so repeats over the same tables give the same bits.
#include <hip/hip_runtime.h>

#include "block_scan.h"
#include "kernels.h"
#include "pair_rules.h"

namespace elemdp {

namespace {
// two neighbouring columns of a row in one 16-byte load (rows start on 8-byte boundaries only)
typedef double dbl2 __attribute__((ext_vector_type(2)));
typedef dbl2 dbl2_a8 __attribute__((aligned(8)));

}  // namespace

// one lane per cell (i fastest, so that neighbouring lanes read neighbouring rows); grid (cells / kThreads, G)
__global__ __launch_bounds__(kThreads) void k4_pairs(PairArgs a) {
  const int g = blockIdx.y;
  const int n = a.idx[g];
  if (a.skip_flagged && a.seq_out[(size_t)n * a.out_stride + 4] != 0.) return;
  const SeqPlan p = a.plans[n];
  const int L = p.L, W = p.W;
  const int t = blockIdx.x * kThreads + threadIdx.x;
  if (t >= (L + 1) * (W + 1)) return;
  const int d = t / (L + 1), i = t - d * (L + 1);
  double v = 0.;
  if (i + d <= L && pair_kept(a.okbits + p.bits_base, i, d, W)) {
    const uint32_t cells = (uint32_t)(W + 1) * (uint32_t)(L + 1);
    const uint32_t row = (uint32_t)a.p_cs * cells + ((uint32_t)d * (uint32_t)(L + 1) + (uint32_t)i) * (uint32_t)a.p_rs;
    const double* in = a.band_in + (size_t)g * a.band_stride + row;
    const double* out = a.band_out + (size_t)g * a.band_stride + row;
    const PairLin r{1. / a.zs[4 * g]};
    double acc = 0.;
    int c = 0;
    for (; c + 1 < a.ncol; c += 2) {
      const dbl2 x = *reinterpret_cast<const dbl2_a8*>(in + c), y = *reinterpret_cast<const dbl2_a8*>(out + c);
      acc += r.term(x.x, y.x);
      acc += r.term(x.y, y.y);
    }
    if (c < a.ncol) acc += r.term(in[c], out[c]);
    v = r.finish(acc);
  }
  a.P[(size_t)g * a.p_stride + (size_t)i * (W + 1) + d] = v;
}

// one workgroup per sequence: unpaired(p), then the pairs with P >= min_prob in (i, j) order into the sequence's staging range
__global__ __launch_bounds__(kThreads) void k_pair_seq(PairArgs a) {
  __shared__ int64_t s_scan[kThreads];
  const int g = blockIdx.x, tid = threadIdx.x;
  const int n = a.idx[g];
  if (a.skip_flagged && a.seq_out[(size_t)n * a.out_stride + 4] != 0.) return;
  const SeqPlan p = a.plans[n];
  const int L = p.L, W = p.W;
  const uint32_t* ok = a.okbits + p.bits_base;
  const double* P = a.P + (size_t)g * a.p_stride;
  for (int q = tid; q < L; q += kThreads) a.unpaired[p.seq_base + q] = pair_unpaired(P, ok, L, W, q);
  const int64_t k0 = a.koff[n];
  int64_t base = 0;
  for (int r0 = 0; r0 <= L; r0 += kThreads) {
    const int i = r0 + tid;
    const int dmax = i <= L ? min(W, L - i) : 0;
    int64_t c = 0;
    for (int d = 1; d <= dmax; ++d)
      if (pair_kept(ok, i, d, W) && P[(size_t)i * (W + 1) + d] >= a.min_prob) ++c;
    int64_t total;
    int64_t at = k0 + base + block_exclusive(c, s_scan, &total);
    for (int d = 1; d <= dmax; ++d) {
      const double v = P[(size_t)i * (W + 1) + d];
      if (pair_kept(ok, i, d, W) && v >= a.min_prob) { a.st_i[at] = i; a.st_j[at] = i + d; a.st_p[at] = v; ++at; }
    }
    base += total;
  }
  if (tid == 0) a.cnt[n] = base;
}

// kept cells of sequence blockIdx.x (an upper bound of its list)
__global__ __launch_bounds__(kThreads) void k_pair_kept(const SeqPlan* plans, const uint32_t* okbits, int64_t* kept) {
  __shared__ int64_t s_scan[kThreads];
  const SeqPlan p = plans[blockIdx.x];
  const int L = p.L, W = p.W, nc = (L + 1) * (W + 1);
  int64_t c = 0;
  for (int t = threadIdx.x; t < nc; t += kThreads) {
    const int i = t / (W + 1), d = t - i * (W + 1);
    if (i + d <= L && pair_kept(okbits + p.bits_base, i, d, W)) ++c;
  }
  int64_t total;
  block_exclusive(c, s_scan, &total);
  if (threadIdx.x == 0) kept[blockIdx.x] = total;
}

// one workgroup: off[k] = sum of cnt[0 .. k), off[n] = the total
__global__ __launch_bounds__(kThreads) void k_pair_prefix(const int64_t* cnt, int n, int64_t* off) {
  __shared__ int64_t s_scan[kThreads];
  const int per = (n + kThreads - 1) / kThreads;
  const int k0 = min(n, (int)threadIdx.x * per), k1 = min(n, k0 + per);
  int64_t c = 0;
  for (int k = k0; k < k1; ++k) c += cnt[k];
  int64_t total;
  int64_t at = block_exclusive(c, s_scan, &total);
  for (int k = k0; k < k1; ++k) { off[k] = at; at += cnt[k]; }
  if (threadIdx.x == 0) off[n] = total;
}

// grid (n): the staging range of batch index blockIdx.x into its place in the batch list (the lists of the pair, conditional and
// stem calls: which columns a list has is uniform over the launch)
__global__ __launch_bounds__(kThreads) void k_list_scatter(ListCols c) {
  const int n = blockIdx.x;
  const int64_t m = c.cnt[n], src = c.koff[n] * c.mult, dst = c.off[n];
  for (int64_t t = threadIdx.x; t < m; t += kThreads) {
    c.seq[dst + t] = n; c.i[dst + t] = c.st_i[src + t]; c.j[dst + t] = c.st_j[src + t];
    c.v[0][dst + t] = c.st_v[0][src + t];
    if (c.st_v[1]) c.v[1][dst + t] = c.st_v[1][src + t];
    if (c.st_k) c.k[dst + t] = c.st_k[src + t];
  }
}

hipError_t launch_pair_cells(const PairArgs& a, int G, int cells_max, hipStream_t st) {
  if (G <= 0) return hipSuccess;
  hipLaunchKernelGGL(k4_pairs, dim3((cells_max + kThreads - 1) / kThreads, G), dim3(kThreads), 0, st, a);
  return hipGetLastError();
}
hipError_t launch_pair_seq(const PairArgs& a, int G, hipStream_t st) {
  if (G <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_pair_seq, dim3(G), dim3(kThreads), 0, st, a);
  return hipGetLastError();
}
hipError_t launch_pair_kept(const SeqPlan* plans, const uint32_t* okbits, int n, int64_t* kept, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_pair_kept, dim3(n), dim3(kThreads), 0, st, plans, okbits, kept);
  return hipGetLastError();
}
hipError_t launch_pair_prefix(const int64_t* cnt, int n, int64_t* off, hipStream_t st) {
  hipLaunchKernelGGL(k_pair_prefix, dim3(1), dim3(kThreads), 0, st, cnt, n, off);
  return hipGetLastError();
}
hipError_t launch_list_scatter(const ListCols& c, int n, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_list_scatter, dim3(n), dim3(kThreads), 0, st, c);
  return hipGetLastError();
}

}  // namespace elemdp
