// access_kernels.hip -- accessibility under the motif model (rule in access_rules.h).  k_access_chains runs on the
// compact tables of the scan's first sum pass (launch_lin_scan_group, SCAN_PASS_START), right behind it on the same slots and
// stream, before the next group of the stream reuses them.  One wave per unit (term, position): the workgroup's four waves take
// four positions of one term.  Lane = entry of the state vector, both vectors and the unit's U sums in the wave's slice of
// LDS: no per-lane array, any state count (the slice is sized at the launch).  k_access_seq, one workgroup per sequence, adds the
// four terms of every window in a fixed order, clamps and writes the NaN tail; it serves the log-space form too, whose planes the
// fused scan kernel writes (DpArgs::acc).  No atomics: every sum has a fixed order, so repeats over the same tables give the same
// bits.  A sequence the range check flagged is left to the log-space form.
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "lin_views.h"
#include "access_rules.h"
#include "lin_params.h"

namespace elemdp {

constexpr int kAccWaves = kThreads / 64;   // units per workgroup

// the 64 lanes of a wave on one unit (every branch around a call is uniform over the wave: it depends on the unit alone)
struct WaveLanes {
  int l;
  __device__ int lane() const { return l; }
  __device__ int n() const { return 64; }
  __device__ void sync() const {
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  }
  __device__ double sum(double v) const {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
  }
  __device__ bool any(bool b) const { return __any(b ? 1 : 0) != 0; }
  __device__ double scan(double v) const {
    for (int o = 1; o < 64; o <<= 1) {
      const double u = __shfl_up(v, o, 64);
      if (l >= o) v += u;
    }
    return v;
  }
  __device__ double last(double v) const { return __shfl(v, 63, 64); }
  template <class P> __device__ uint64_t mask(int n, P pred) const { return __ballot(l < n && pred(l) ? 1 : 0); }
};

// the terms in launch order, the heavy ones first: a workgroup's waves take four positions of one term, so the workgroups of the
// two light terms leave their CU early
__device__ __forceinline__ int acc_term_of(int k) { return k == 0 ? ACC_2 : k == 1 ? ACC_M : k == 2 ? ACC_O : ACC_L; }

// dynamic LDS of k_access_chains (bytes): the linear parameter block, kAccWaves slices of 2 n_vec + 2 U doubles (two vectors, the
// unit's sums, the position weights of the unit's bases), the small part of the automaton blob (n_ints of them, 0: left in global
// memory), kAccWaves x U base codes
__host__ __device__ inline size_t acc_slice(int n_vec, int U) { return 2 * (size_t)n_vec + 2 * (size_t)U; }
__host__ __device__ inline size_t acc_lds_bytes(int n_lin, int n_vec, int U, int n_ints) {
  return 8 * ((size_t)n_lin + kAccWaves * acc_slice(n_vec, U)) + 4 * (size_t)n_ints + (size_t)kAccWaves * ((U + 7) & ~7);
}

// grid (4 ceil((L + 1) / kAccWaves), G): block k * nb + r is term acc_term_of(k), positions kAccWaves r ..
// Every step of a chain reads per-state attributes, a transition list and an emission weight; from global memory these are
// dependent loads on the critical path of every step.  So the workgroup stages the small part of the automaton blob (the column
// map of the compact tables with it) and the linear parameter block, and a wave the base codes and position weights of the U bases
// its unit emits; a step then waits for LDS alone, and the outside entry of the step is in flight next to it.
__global__ __launch_bounds__(kThreads) void k_access_chains(LinArgs a, AccessArgs c, int n_vec, int n_ints, int n_lin) {
  extern __shared__ __align__(16) unsigned char s_raw[];
  __shared__ AutomatonLayout s_lay;
  {
    const int32_t* src = reinterpret_cast<const int32_t*>(a.layp);
    int32_t* dst = reinterpret_cast<int32_t*>(&s_lay);
    for (int t = threadIdx.x; t < (int)(sizeof(AutomatonLayout) / sizeof(int32_t)); t += kThreads) dst[t] = src[t];
  }
  const int U = c.U;
  double* llin = reinterpret_cast<double*>(s_raw);
  double* slices = llin + n_lin;
  int32_t* blob = reinterpret_cast<int32_t*>(slices + kAccWaves * acc_slice(n_vec, U));
  uint8_t* lseq = reinterpret_cast<uint8_t*>(blob + n_ints);
  for (int t = threadIdx.x; t < n_lin; t += kThreads) llin[t] = a.lin[t];
  for (int t = threadIdx.x; t < n_ints; t += kThreads) blob[t] = a.ints[t];
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
  const int L = v.q.L;
  const int nb = gridDim.x / ACC_TERMS;
  const int term = acc_term_of(blockIdx.x / nb);
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int x = (blockIdx.x % nb) * kAccWaves + wave;
  if (x > L) return;
  const WaveLanes ln{(int)(threadIdx.x & 63)};
  double* row = c.T + (size_t)g * c.t_stride + (size_t)term * c.plane + (size_t)x * U;
  if (!((c.terms >> term) & 1)) {   // (option access_terms: the term is left out)
    for (int w = ln.l; w < U; w += 64) row[w] = 0.;
    return;
  }
  double* v0 = slices + (size_t)wave * acc_slice(n_vec, U);
  double* v1 = v0 + n_vec;
  double* sums = v1 + n_vec;
  double* lews = sums + U;
  uint8_t* lsq = lseq + (size_t)wave * ((U + 7) & ~7);
  // the bases the unit emits: x .. x + U - 1 behind a start, x - U .. x - 1 in front of an end
  const int p0 = term == ACC_M ? (x > U ? x - U : 0) : x;
  for (int t = ln.l; t < U; t += 64) {
    const int p = p0 + t;
    lsq[t] = p < L ? v.q.seq[p] : (uint8_t)0;
    lews[t] = p < L ? v.q.ews[p] : 1.;
  }
  ln.sync();
  // (the staged arrays keep their own origin, handed to the weights as p0: a pointer moved in front of an LDS array leaves the LDS
  // aperture once the compiler does the subtraction on the 32-bit LDS offset)
  SeqView q = v.q;
  q.seq = lsq; q.ews = lews;
  const AccLin f(1. / v.zs[0], p0);
  access_unit(f, ln, v.m, q, v.in, v.out, term, x, U, v0, v1, sums);
  ln.sync();
  for (int w = ln.l; w < U; w += 64) row[w] = sums[w];
}

// one workgroup per sequence, the L U windows in tiles of kThreads
__global__ __launch_bounds__(kThreads) void k_access_seq(AccessArgs c) {
  const int g = blockIdx.x, tid = threadIdx.x;
  const int n = c.idx[g];
  if (c.skip_flagged && c.seq_out[(size_t)n * c.out_stride + 4] != 0.) return;
  const SeqPlan p = c.plans[n];
  const int L = p.L, U = c.U;
  double* acc = c.access + (size_t)U * p.seq_base;
  const double* T = c.T + (size_t)g * c.t_stride;
  for (int t0 = 0; t0 < L * U; t0 += kThreads) {
    const int t = t0 + tid;
    if (t >= L * U) break;
    const int pos = t / U, w = t - pos * U + 1;
    acc[t] = c.no_rss ? access_value_no_rss(L, pos, w) : access_value(T, c.plane, L, U, pos, w);
  }
}

hipError_t launch_access_chains(const LinArgs& a, const AccessArgs& c, int G, int Lmax, int n_vec, hipStream_t st) {
  if (G <= 0) return hipSuccess;
  constexpr size_t kLdsMax = 60 * 1024;   // (with the static part below the 64 KiB a workgroup may ask for)
  const int n_lin = kLinEth + a.lay.n_theta;   // (tau, the per-base scales, exp(theta): what lw_right / lw_left read)
  int n_ints = a.lay.n_small;
  if (acc_lds_bytes(n_lin, n_vec, c.U, n_ints) > kLdsMax) n_ints = 0;   // (a large automaton: its blob stays in global memory)
  const size_t lds = acc_lds_bytes(n_lin, n_vec, c.U, n_ints);
  if (lds > kLdsMax) return hipErrorInvalidValue;   // (some thousand interval states: no such pattern is accepted)
  const int nb = (Lmax + 1 + kAccWaves - 1) / kAccWaves;
  hipLaunchKernelGGL(k_access_chains, dim3(ACC_TERMS * nb, G), dim3(kThreads), lds, st, lin_in_world(a), c, n_vec, n_ints, n_lin);
  return hipGetLastError();
}
hipError_t launch_access_seq(const AccessArgs& c, int G, hipStream_t st) {
  if (G <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_access_seq, dim3(G), dim3(kThreads), 0, st, c);
  return hipGetLastError();
}

}  // namespace elemdp
