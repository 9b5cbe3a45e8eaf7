// helix_kernels.hip -- helix posteriors under the motif model (rule in helix_rules.h).  The kernels run on the compact
// tables of the scan's first sum pass (launch_lin_scan_group, SCAN_PASS_START) and the P plane of launch_pair_cells, right behind
// them on the same slots and stream, before the next group of the stream reuses them.
//   k_helix_units   one workgroup per sequence: the kept cells whose P reaches min_prob become the slot's units, in (i, d) order (the
//                   count / prefix scheme of k_pair_seq).  No wave is launched for a cell of the band that is no unit.
//   k_helix_chains  one wave per unit, lane = state, states beyond 64 strided over the lanes, the two vectors in the wave's slice
//                   of LDS: no per-lane array, any state count.  A workgroup's four waves stride over the units of its sequence,
//                   then over the stems of its caller-given structure: the same chain with no bound and no threshold.  The small
//                   part of the automaton blob and the linear parameter block are staged in LDS once per workgroup.
//   k_helix_seq     one workgroup per sequence: the entries (i, j, len) with min_len <= len <= the length its unit reached, in
//                   (i, j, len) order, into the sequence's staging range; the batch list behind the prefix over the counts is
//                   k_list_scatter's (pair_kernels.hip).  It serves the log-space form too, whose units the fused scan kernel
//                   writes (DpArgs::hlx).
// No atomics, plain vector stores: every sum has a fixed order, so repeats over the same tables give the same bits.  A sequence the
// range check flagged is left to the log-space form.
#include <hip/hip_runtime.h>

#include "block_scan.h"
#include "kernels.h"
#include "lin_params.h"
#include "lin_views.h"
#include "helix_rules.h"

namespace elemdp {

constexpr int kHelixWaves = kThreads / 64;   // units in flight per workgroup

// the 64 lanes of a wave on one unit (every branch around a call is uniform over the wave: it depends on the unit alone): what the
// chain needs of the wave policy of access_kernels.hip, and helix_first below
struct HelixWave {
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
};
__device__ inline double helix_first(const HelixWave&, double v) { return __shfl(v, 0, 64); }

// a unit is picked where P reaches min_prob less a margin of rounding: P is the serial sum of k4_pairs, the chain's own H(1) -- the
// same terms over a tree of lanes -- then decides whether the cell is listed
__device__ __forceinline__ double helix_pick_bound(double min_prob) { return min_prob * (1. - 0x1p-30); }

// grid (G): the units of the sequence idx[g]
__global__ __launch_bounds__(kThreads) void k_helix_units(HelixArgs c) {
  __shared__ int64_t s_scan[kThreads];
  const int g = blockIdx.x, tid = threadIdx.x;
  const int n = c.idx[g];
  if (c.skip_flagged && c.seq_out[(size_t)n * c.out_stride + 4] != 0.) return;
  const SeqPlan p = c.plans[n];
  const int L = p.L, W = p.W;
  const uint32_t* ok = c.okbits + p.bits_base;
  const double* P = c.P + (size_t)g * c.p_stride;
  int32_t* ui = c.ui + (size_t)g * c.u_stride;
  int32_t* ud = c.ud + (size_t)g * c.u_stride;
  const double bound = helix_pick_bound(c.min_prob);
  int64_t base = 0;
  for (int r0 = 0; r0 <= L; r0 += kThreads) {
    const int i = r0 + tid;
    const int dmax = i <= L ? min(W, L - i) : 0;
    int64_t m = 0;
    for (int d = 2; d <= dmax; ++d)
      if (pair_kept(ok, i, d, W) && P[(size_t)i * (W + 1) + d] >= bound) ++m;
    int64_t total;
    int64_t at = base + block_exclusive(m, s_scan, &total);
    for (int d = 2; d <= dmax; ++d)
      if (pair_kept(ok, i, d, W) && P[(size_t)i * (W + 1) + d] >= bound) { ui[at] = i; ud[at] = d; ++at; }
    base += total;
  }
  if (tid == 0) c.n_units[g] = (int32_t)base;
}

// dynamic LDS of k_helix_chains (bytes): the linear parameter block, kHelixWaves slices of two vectors, the small part of the
// automaton blob (n_ints of them, 0: left in global memory)
__host__ __device__ inline size_t helix_lds_bytes(int n_lin, int S, int n_ints) {
  return 8 * ((size_t)n_lin + (size_t)kHelixWaves * 2 * (size_t)S) + 4 * (size_t)n_ints;
}

// grid (nb, G): the waves of the nb workgroups of slot g stride over its units, then over the stems of its sequence
__global__ __launch_bounds__(kThreads) void k_helix_chains(LinArgs a, HelixArgs c, int n_ints, int n_lin) {
  extern __shared__ __align__(16) unsigned char s_raw[];
  __shared__ AutomatonLayout s_lay;
  {
    const int32_t* src = reinterpret_cast<const int32_t*>(a.layp);
    int32_t* dst = reinterpret_cast<int32_t*>(&s_lay);
    for (int t = threadIdx.x; t < (int)(sizeof(AutomatonLayout) / sizeof(int32_t)); t += kThreads) dst[t] = src[t];
  }
  double* llin = reinterpret_cast<double*>(s_raw);
  for (int t = threadIdx.x; t < n_lin; t += kThreads) llin[t] = a.lin[t];
  __syncthreads();
  const int S = s_lay.S;
  double* slices = llin + n_lin;
  int32_t* blob = reinterpret_cast<int32_t*>(slices + (size_t)kHelixWaves * 2 * S);
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
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const HelixWave ln{(int)(threadIdx.x & 63)};
  double* v0 = slices + (size_t)wave * 2 * S;
  double* v1 = v0 + S;
  const HelixLin f(1. / v.zs[0]);
  const int nu = c.st_i ? c.n_units[g] : 0;
  const int64_t s0 = c.soff ? c.soff[v.n] : 0;
  const int ns = c.soff ? (int)(c.soff[v.n + 1] - s0) : 0;
  const int32_t* ui = c.ui + (size_t)g * c.u_stride;
  const int32_t* ud = c.ud + (size_t)g * c.u_stride;
  int32_t* nlen = c.nlen + (size_t)g * c.u_stride;
  double* X = c.X + (size_t)g * c.u_stride * (size_t)c.max_len;
  for (int u = blockIdx.x * kHelixWaves + wave; u < nu + ns; u += gridDim.x * kHelixWaves) {
    if (u < nu) {
      const HelixRun r = helix_chain(f, ln, v.m, v.q, v.in, v.out, ui[u], ud[u], c.max_len, c.min_prob, v0, v1, X + helix_at(c.max_len, u, 1));
      if (ln.l == 0) nlen[u] = r.n;
    } else {
      const int64_t t = s0 + (u - nu);
      const double h = helix_stem(f, ln, v.m, v.q, v.in, v.out, c.s_i[t], c.s_d[t], c.s_len[t], v0, v1);
      if (ln.l == 0) c.s_p[t] = h;
    }
    ln.sync();   // (the next unit's start vector overwrites v0)
  }
}

// grid (G): the list entries of the sequence idx[g], units in tiles of kThreads lanes
__global__ __launch_bounds__(kThreads) void k_helix_seq(HelixArgs c) {
  __shared__ int64_t s_scan[kThreads];
  const int g = blockIdx.x, tid = threadIdx.x;
  const int n = c.idx[g];
  if (c.skip_flagged && c.seq_out[(size_t)n * c.out_stride + 4] != 0.) return;
  const int nu = c.no_rss ? 0 : c.n_units[g];   // (no secondary structure in the model: no unit was written, nothing is read)
  const int32_t* ui = c.ui + (size_t)g * c.u_stride;
  const int32_t* ud = c.ud + (size_t)g * c.u_stride;
  const int32_t* nlen = c.nlen + (size_t)g * c.u_stride;
  const double* X = c.X + (size_t)g * c.u_stride * (size_t)c.max_len;
  const int64_t k0 = c.koff[n] * (int64_t)(c.max_len - c.min_len + 1);
  int64_t base = 0;
  for (int r0 = 0; r0 < nu; r0 += kThreads) {
    const int r = r0 + tid;
    const int top = r < nu ? nlen[r] : 0;
    const int64_t m = top >= c.min_len ? top - c.min_len + 1 : 0;
    int64_t total;
    int64_t at = k0 + base + block_exclusive(m, s_scan, &total);
    if (m > 0) {
      const int i = ui[r], j = i + ud[r];
      for (int k = c.min_len; k <= top; ++k) {
        c.st_i[at] = i; c.st_j[at] = j; c.st_k[at] = (uint8_t)k; c.st_h[at] = X[helix_at(c.max_len, r, k)];
        ++at;
      }
    }
    base += total;
  }
  if (tid == 0) c.cnt[n] = base;
}

hipError_t launch_helix_units(const HelixArgs& c, int G, hipStream_t st) {
  if (G <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_helix_units, dim3(G), dim3(kThreads), 0, st, c);
  return hipGetLastError();
}
hipError_t launch_helix_chains(const LinArgs& a, const HelixArgs& c, int G, int cells_max, hipStream_t st) {
  if (G <= 0 || cells_max <= 0) return hipSuccess;
  constexpr size_t kLdsMax = 60 * 1024;   // (with the static part below the 64 KiB a workgroup may ask for)
  const int n_lin = kLinEth + a.lay.n_theta;   // (tau, the per-base scales, exp(theta): what lw_pair reads)
  int n_ints = a.lay.n_small;
  if (helix_lds_bytes(n_lin, a.lay.S, n_ints) > kLdsMax) n_ints = 0;   // (a large automaton: its blob stays in global memory)
  const size_t lds = helix_lds_bytes(n_lin, a.lay.S, n_ints);
  if (lds > kLdsMax) return hipErrorInvalidValue;
  // (the units of a sequence are a small part of its cells; a sequence's workgroups stride over them)
  const int nb = std::max(1, std::min(16, (cells_max + 64 * kHelixWaves - 1) / (64 * kHelixWaves)));
  hipLaunchKernelGGL(k_helix_chains, dim3(nb, G), dim3(kThreads), lds, st, lin_in_world(a), c, n_ints, n_lin);
  return hipGetLastError();
}
hipError_t launch_helix_seq(const HelixArgs& c, int G, hipStream_t st) {
  if (G <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_helix_seq, dim3(G), dim3(kThreads), 0, st, c);
  return hipGetLastError();
}

}  // namespace elemdp
