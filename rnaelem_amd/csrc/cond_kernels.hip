// cond_kernels.hip -- motif-conditional pair posteriors (rule in cond_rules.h): the pair reduction of one world over
// the compact tables behind that world's outside sweep (k4_cond), the per-sequence pass over both worlds -- unpaired vectors,
// exist_prob, shift and the compaction with two probability columns (k_cond_seq).  The batch list in (sequence, i, j) order is
// built by the counts, prefixes and scatter of pair_kernels.hip.  No atomics: every sum has a fixed order, so repeats over the
// same tables give the same bits.
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "cond_rules.h"

namespace elemdp {

namespace {
typedef double dbl2 __attribute__((ext_vector_type(2)));
typedef dbl2 dbl2_a8 __attribute__((aligned(8)));

__device__ __forceinline__ CondZ cond_z(const CondArgs& a, int g) {
  return CondZ{a.z[4 * g], a.z[4 * g + 1], a.z[4 * g + 2], a.z_log != 0};
}

// exclusive prefix over the workgroup (kThreads lanes); returns the workgroup's total through *total
__device__ int64_t block_exclusive(int64_t v, int64_t* s, int64_t* total) {
  const int tid = threadIdx.x;
  s[tid] = v;
  __syncthreads();
  for (int off = 1; off < kThreads; off <<= 1) {
    const int64_t u = tid >= off ? s[tid - off] : 0;
    __syncthreads();
    s[tid] += u;
    __syncthreads();
  }
  const int64_t incl = s[tid];
  *total = s[kThreads - 1];
  __syncthreads();
  return incl - v;
}
}  // namespace

// one lane per cell (i fastest, so that neighbouring lanes read neighbouring rows); grid (cells / kThreads, G).  The outside
// sweep of an empty world left the sequence alone: its outside rows are not read.
__global__ __launch_bounds__(kThreads) void k4_cond(CondArgs a, int world) {
  const int g = blockIdx.y;
  const int n = a.idx[g];
  if (a.skip_flagged && a.seq_out[(size_t)n * a.out_stride + 4] != 0.) return;
  const SeqPlan p = a.plans[n];
  const int L = p.L, W = p.W;
  const int t = blockIdx.x * kThreads + threadIdx.x;
  if (t >= (L + 1) * (W + 1)) return;
  const int d = t / (L + 1), i = t - d * (L + 1);
  const CondZ z = cond_z(a, g);
  double v = 0.;
  if (!z.empty(world) && i + d <= L && pair_kept(a.okbits + p.bits_base, i, d, W)) {
    const uint32_t cells = (uint32_t)(W + 1) * (uint32_t)(L + 1);
    const uint32_t row = (uint32_t)a.p_cs * cells + ((uint32_t)d * (uint32_t)(L + 1) + (uint32_t)i) * (uint32_t)a.p_rs;
    const double* in = a.band_in + (size_t)g * a.band_stride + row;
    const double* out = a.band_out + (size_t)g * a.band_stride + row;
    const PairLin r{1. / z.of(world)};
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
  (world == COND_MOTIF ? a.P[0] : a.P[1])[(size_t)g * a.p_stride + (size_t)i * (W + 1) + d] = v;
}

// one workgroup per sequence, the rows i in tiles of kThreads: both unpaired vectors, exist_prob, the shift (rows summed in
// increasing i by one lane), then the cells with max(P_motif, P_none) >= min_prob in (i, j) order into the sequence's staging range
__global__ __launch_bounds__(kThreads) void k_cond_seq(CondArgs a) {
  __shared__ int64_t s_scan[kThreads];
  __shared__ double s_row[kThreads];
  __shared__ double s_shift;
  const int g = blockIdx.x, tid = threadIdx.x;
  const int n = a.idx[g];
  if (a.skip_flagged && a.seq_out[(size_t)n * a.out_stride + 4] != 0.) return;
  const SeqPlan p = a.plans[n];
  const int L = p.L, W = p.W;
  const uint32_t* ok = a.okbits + p.bits_base;
  const double* P0 = a.P[0] + (size_t)g * a.p_stride;
  const double* P1 = a.P[1] + (size_t)g * a.p_stride;
  const CondZ z = cond_z(a, g);
  for (int q = tid; q < L; q += kThreads) {
    a.unpaired[0][p.seq_base + q] = pair_unpaired(P0, ok, L, W, q);
    a.unpaired[1][p.seq_base + q] = pair_unpaired(P1, ok, L, W, q);
  }
  if (tid == 0) s_shift = 0.;
  const int64_t k0 = a.koff[n];
  int64_t base = 0;
  for (int r0 = 0; r0 <= L; r0 += kThreads) {
    const int i = r0 + tid;
    const int dmax = i <= L ? min(W, L - i) : 0;
    s_row[tid] = cond_shift_row(P0, P1, ok, W, i, dmax);
    int64_t c = 0;
    for (int d = 1; d <= dmax; ++d)
      if (pair_kept(ok, i, d, W) && cond_listed(P0[(size_t)i * (W + 1) + d], P1[(size_t)i * (W + 1) + d], a.min_prob)) ++c;
    int64_t total;
    int64_t at = k0 + base + block_exclusive(c, s_scan, &total);   // (its barriers also order s_row and s_shift)
    if (tid == 0) {
      double acc = s_shift;
      const int rows = min(kThreads, L + 1 - r0);
      for (int r = 0; r < rows; ++r) acc += s_row[r];
      s_shift = acc;
    }
    for (int d = 1; d <= dmax; ++d) {
      const double v0 = P0[(size_t)i * (W + 1) + d], v1 = P1[(size_t)i * (W + 1) + d];
      if (pair_kept(ok, i, d, W) && cond_listed(v0, v1, a.min_prob)) {
        a.st_i[at] = i; a.st_j[at] = i + d; a.st_p[0][at] = v0; a.st_p[1][at] = v1;
        ++at;
      }
    }
    base += total;
    __syncthreads();   // (lane 0 has read s_row before the next tile overwrites it)
  }
  if (tid == 0) {
    a.cnt[n] = base;
    a.exist[n] = z.exist();
    a.shift[n] = (z.empty(COND_MOTIF) || z.empty(COND_NONE)) ? __builtin_nan("") : s_shift;
  }
}

hipError_t launch_cond_cells(const CondArgs& a, int world, int G, int cells_max, hipStream_t st) {
  if (G <= 0) return hipSuccess;
  hipLaunchKernelGGL(k4_cond, dim3((cells_max + kThreads - 1) / kThreads, G), dim3(kThreads), 0, st, a, world);
  return hipGetLastError();
}
hipError_t launch_cond_seq(const CondArgs& a, int G, hipStream_t st) {
  if (G <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_cond_seq, dim3(G), dim3(kThreads), 0, st, a);
  return hipGetLastError();
}

}  // namespace elemdp
