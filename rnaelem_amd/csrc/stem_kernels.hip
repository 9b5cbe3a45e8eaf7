// stem_kernels.hip -- pair posteriors by motif node pair and the pair counts behind a stem logo (rule in
// stem_rules.h).  k_stem_cells runs on the compact tables of the scan's first sum pass (launch_lin_scan_group, SCAN_PASS_START),
// right behind it on the same slots and stream, before the next group of the stream reuses them.
//   k_stem_cells   one lane per cell, i fastest as k4_pairs, so neighbouring lanes read neighbouring rows and write neighbouring
//                  doubles of the scratch.  The slot lists, the small part of the automaton blob and the linear parameter block are
//                  staged in LDS once per workgroup.  The loop is slot-major over the grouped transition list: one running sum per
//                  lane at a time, no per-lane array, any K.
//   k_stem_counts  one workgroup per sequence, one lane per (slot, left base, right base).  The mask and the bases of the sequence
//                  are staged in LDS; the lanes walk the set bits of the mask together, in (i, d) order, as scalar work, and a lane
//                  only adds where the two bases are its own.  It serves the log-space form too, whose Q the fused scan kernel
//                  writes (DpArgs::stm).
//   k_stem_seq     one workgroup per sequence: the entries with q >= min_prob in (i, j, slot) order into the sequence's staging
//                  range (the scheme of k_pair_seq); the batch list behind the prefix over the counts is k_list_scatter's
//                  (pair_kernels.hip).
// No atomics: every sum has a fixed order, so repeats over the same tables give the same bits.  A sequence the range check flagged
// is left to the log-space form.
#include <hip/hip_runtime.h>

#include "block_scan.h"
#include "kernels.h"
#include "lin_params.h"
#include "lin_views.h"
#include "stem_rules.h"

namespace elemdp {

// dynamic LDS of k_stem_cells (bytes): the linear parameter block, the small part of the automaton blob, the slot lists (either
// int count 0: left in global memory)
__host__ __device__ inline size_t stem_lds_bytes(int n_lin, int n_ints, int n_list) {
  return 8 * (size_t)n_lin + 4 * ((size_t)n_ints + (size_t)n_list);
}

// grid (ceil(cells / kThreads), G)
__global__ __launch_bounds__(kThreads) void k_stem_cells(LinArgs a, StemArgs c, int n_ints, int n_lin, int n_list) {
  extern __shared__ __align__(16) unsigned char s_raw[];
  __shared__ AutomatonLayout s_lay;
  {
    const int32_t* src = reinterpret_cast<const int32_t*>(a.layp);
    int32_t* dst = reinterpret_cast<int32_t*>(&s_lay);
    for (int t = threadIdx.x; t < (int)(sizeof(AutomatonLayout) / sizeof(int32_t)); t += kThreads) dst[t] = src[t];
  }
  double* llin = reinterpret_cast<double*>(s_raw);
  int32_t* blob = reinterpret_cast<int32_t*>(llin + n_lin);
  int32_t* llist = blob + n_ints;
  for (int t = threadIdx.x; t < n_lin; t += kThreads) llin[t] = a.lin[t];
  for (int t = threadIdx.x; t < n_ints; t += kThreads) blob[t] = a.ints[t];
  for (int t = threadIdx.x; t < n_list; t += kThreads) llist[t] = c.lists[t];
  __syncthreads();
  const int g = blockIdx.y;
  LViews v(s_lay);
  make_lviews(a, g, v);
  if (v.row[4] != 0.) return;   // (outside the double range: the log-space form of the fused scan kernel covers it)
  v.m.lin = llin;
  if (n_ints > 0) {
    v.m.ints = blob;
    v.in.cm = v.out.cm = blob + s_lay.tab_cmap;
  }
  const int L = v.q.L, W = v.q.W;
  if (blockIdx.x == 0 && threadIdx.x == 0) c.has[v.n] = 1;
  const int t = blockIdx.x * kThreads + threadIdx.x;
  if (t >= (L + 1) * (W + 1)) return;
  const int d = t / (L + 1), i = t - d * (L + 1);
  if (i + d > L) return;
  const StemLin f(1. / v.zs[0]);
  const StemLists sl{n_list > 0 ? llist : c.lists, c.K, SP_ALL};
  double* X = c.X + (size_t)g * c.x_stride;
  if (d >= 2 && v.q.pair_ok(i, d)) {
    for (int k = 0; k < c.K; ++k) X[stem_at(L, W, k, i, d)] = stem_cell(f, sl, v.m, v.q, v.in, v.out, d, i, k);
  } else {
    for (int k = 0; k < c.K; ++k) X[stem_at(L, W, k, i, d)] = 0.;
  }
}

// dynamic LDS of k_stem_counts (bytes): the pair mask of the sequence, then its bases
__host__ __device__ inline size_t stem_counts_lds_bytes(int Lmax, int Wmax) {
  return 4 * ((((size_t)Lmax + 1) * ((size_t)Wmax + 1) + 31) / 32) + 4 * (((size_t)Lmax + 3) / 4);
}

// grid (G): the counts of the sequence idx[g].  staged: the mask and the bases of the sequence are read from LDS (else they do
// not fit: from global memory).
__global__ __launch_bounds__(kThreads) void k_stem_counts(StemArgs c, int staged) {
  extern __shared__ __align__(16) unsigned char s_raw[];
  const int g = blockIdx.x;
  const int n = c.idx[g];
  if (c.skip_flagged && c.seq_out[(size_t)n * c.out_stride + 4] != 0.) return;
  const SeqPlan p = c.plans[n];
  const int nc = c.K * kStemBlock;
  double* counts = c.counts + (size_t)nc * n;
  if (!c.has[n]) {   // (no parse, or no secondary structure in the model: X is not read)
    for (int t = threadIdx.x; t < nc; t += kThreads) counts[t] = 0.;
    return;
  }
  const uint8_t* seq = c.seq + p.seq_base;
  const uint32_t* ok = c.okbits + p.bits_base;
  if (staged) {
    const int nword = ((p.L + 1) * (p.W + 1) + 31) / 32;
    uint32_t* lok = reinterpret_cast<uint32_t*>(s_raw);
    uint8_t* lseq = reinterpret_cast<uint8_t*>(lok + nword);
    for (int t = threadIdx.x; t < nword; t += kThreads) lok[t] = ok[t];
    for (int t = threadIdx.x; t < p.L; t += kThreads) lseq[t] = seq[t];
    __syncthreads();
    seq = lseq; ok = lok;
  }
  const double* X = c.X + (size_t)g * c.x_stride;
  for (int t = threadIdx.x; t < nc; t += kThreads) counts[t] = stem_count(X, seq, ok, p.L, p.W, t);
}

// grid (G): the entries of the sequence idx[g] with q >= min_prob, rows of kThreads lanes at a time
__global__ __launch_bounds__(kThreads) void k_stem_seq(StemArgs c) {
  __shared__ int64_t s_scan[kThreads];
  const int g = blockIdx.x, tid = threadIdx.x;
  const int n = c.idx[g];
  if (c.skip_flagged && c.seq_out[(size_t)n * c.out_stride + 4] != 0.) return;
  if (!c.has[n]) {   // (no parse, or no secondary structure in the model: no entries, X is not read)
    if (tid == 0) c.cnt[n] = 0;
    return;
  }
  const SeqPlan p = c.plans[n];
  const int L = p.L, W = p.W, K = c.K;
  const uint32_t* ok = c.okbits + p.bits_base;
  const double* X = c.X + (size_t)g * c.x_stride;
  const int64_t k0 = c.koff[n] * K;
  int64_t base = 0;
  for (int r0 = 0; r0 <= L; r0 += kThreads) {
    const int i = r0 + tid;
    const int dmax = i <= L ? min(W, L - i) : 0;
    int64_t m = 0;
    for (int d = 1; d <= dmax; ++d)
      if (pair_kept(ok, i, d, W))
        for (int k = 0; k < K; ++k)
          if (X[stem_at(L, W, k, i, d)] >= c.min_prob) ++m;
    int64_t total;
    int64_t at = k0 + base + block_exclusive(m, s_scan, &total);
    for (int d = 1; d <= dmax; ++d)
      if (pair_kept(ok, i, d, W))
        for (int k = 0; k < K; ++k) {
          const double q = X[stem_at(L, W, k, i, d)];
          if (q >= c.min_prob) { c.st_i[at] = i; c.st_j[at] = i + d; c.st_k[at] = (uint8_t)k; c.st_q[at] = q; ++at; }
        }
    base += total;
  }
  if (tid == 0) c.cnt[n] = base;
}

hipError_t launch_stem_cells(const LinArgs& a, const StemArgs& c, int G, int cells_max, hipStream_t st) {
  if (G <= 0 || cells_max <= 0) return hipSuccess;
  constexpr size_t kLdsMax = 60 * 1024;   // (with the static part below the 64 KiB a workgroup may ask for)
  const int n_lin = kLinEth + a.lay.n_theta;   // (tau, the per-base scales, exp(theta): what lw_pair reads)
  int n_ints = a.lay.n_small, n_list = c.n_list;
  if (stem_lds_bytes(n_lin, n_ints, n_list) > kLdsMax) n_ints = 0;   // (a large automaton: its blob stays in global memory,
  if (stem_lds_bytes(n_lin, n_ints, n_list) > kLdsMax) n_list = 0;   //  then the lists)
  const size_t lds = stem_lds_bytes(n_lin, n_ints, n_list);
  if (lds > kLdsMax) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_stem_cells, dim3((cells_max + kThreads - 1) / kThreads, G), dim3(kThreads), lds, st, lin_in_world(a), c, n_ints, n_lin, n_list);
  return hipGetLastError();
}
hipError_t launch_stem_counts(const StemArgs& c, int G, int Lmax, int Wmax, hipStream_t st) {
  if (G <= 0) return hipSuccess;
  size_t lds = stem_counts_lds_bytes(Lmax, Wmax);
  if (lds > 48 * 1024) lds = 0;   // (a long sequence: its mask stays in global memory)
  hipLaunchKernelGGL(k_stem_counts, dim3(G), dim3(kThreads), lds, st, c, lds > 0 ? 1 : 0);
  return hipGetLastError();
}
hipError_t launch_stem_seq(const StemArgs& c, int G, hipStream_t st) {
  if (G <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_stem_seq, dim3(G), dim3(kThreads), 0, st, c);
  return hipGetLastError();
}

}  // namespace elemdp
