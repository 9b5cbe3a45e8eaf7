// loop_kernels.hip -- loop posteriors under the motif model (rule in loop_rules.h).  The kernels run on the compact
// tables of the scan's first sum pass (launch_lin_scan_group, SCAN_PASS_START), the P plane of launch_pair_cells and the units of
// launch_helix_units (the kept cells whose P reaches the bound, in (i, d) order: the compaction of helix_kernels.hip), right behind
// them on the same slots and stream, before the next group of the stream reuses them.
//   k_loop_unary    one lane per unit: the columns H, S and M of its cell.
//   k_loop_items    one wave per unit: out(E, outer, .) of the unit's outer cell is staged once in the wave's slice of LDS (states
//                   beyond 64 strided over the lanes: no per-lane array, any state count), the lanes stride over the cell's rule-6c
//                   items, each lane walks the quad list for its item and writes T to the slot's scratch at the item's by-outer
//                   position; B and I are the lanes' sums in item order, then a fixed tree over the lanes.  The item weights depend
//                   on the item's energy, so they are formed per item, not staged with out(E).  The small part of the automaton blob
//                   and the linear parameter block are staged in LDS once per workgroup.
//   k_loop_struct   one lane per loop of the caller-given structure of the sequence: the same rule by one lane, no threshold.
//   k_loop_seq      one workgroup per sequence: the counts -- the column sums over the units, lanes strided over the units, then a
//                   fixed tree --, and the entries of both lists into the sequence's staging ranges: a closing entry per unit whose
//                   P reaches min_prob, a two-loop entry per item of a unit whose T reaches it, units in (i, d) order, items in
//                   by-outer order.  It serves the log-space form too, whose units the fused scan kernel writes (DpArgs::lop).
//   k_loop_scatter  the staging ranges into the batch lists behind the prefixes over the counts.
// No atomics, plain vector stores: every sum has a fixed order, so repeats over the same tables give the same bits.  A sequence the
// range check flagged is left to the log-space form.
#include <hip/hip_runtime.h>

#include "block_scan.h"
#include "kernels.h"
#include "lin_params.h"
#include "lin_views.h"
#include "loop_rules.h"

namespace elemdp {

constexpr int kLoopWaves = kThreads / 64;   // units in flight per workgroup of k_loop_items

// dynamic LDS (bytes): the linear parameter block, n_vec state vectors, the small part of the automaton blob (n_ints of them, 0:
// left in global memory)
__host__ __device__ inline size_t loop_lds_bytes(int n_lin, int S, int n_vec, int n_ints) {
  return 8 * ((size_t)n_lin + (size_t)n_vec * (size_t)S) + 4 * (size_t)n_ints;
}

// the staging every kernel on the tables starts with; false: the sequence of the slot is not this form's
__device__ __forceinline__ bool loop_views(const LinArgs& a, AutomatonLayout& s_lay, unsigned char* s_raw, int n_lin, int n_vec,
                                           int n_ints, int g, LViews& v, double** vecs) {
  double* llin = reinterpret_cast<double*>(s_raw);
  for (int t = threadIdx.x; t < n_lin; t += kThreads) llin[t] = a.lin[t];
  const int S = s_lay.S;
  *vecs = llin + n_lin;
  int32_t* blob = reinterpret_cast<int32_t*>(*vecs + (size_t)n_vec * S);
  for (int t = threadIdx.x; t < n_ints; t += kThreads) blob[t] = a.ints[t];
  __syncthreads();
  make_lviews(a, g, v);
  if (v.row[4] != 0.) return false;   // (outside the double range: the log-space form of the fused scan kernel covers it)
  v.m.lin = llin;
  if (n_ints > 0) {
    v.m.ints = blob;
    v.in.cm = v.out.cm = blob + s_lay.tab_cmap;
  }
  return true;
}
__device__ __forceinline__ void loop_stage_layout(const LinArgs& a, AutomatonLayout& s_lay) {
  const int32_t* src = reinterpret_cast<const int32_t*>(a.layp);
  int32_t* dst = reinterpret_cast<int32_t*>(&s_lay);
  for (int t = threadIdx.x; t < (int)(sizeof(AutomatonLayout) / sizeof(int32_t)); t += kThreads) dst[t] = src[t];
  __syncthreads();
}

// grid (nb, G): the lanes of the nb workgroups of slot g stride over its units
__global__ __launch_bounds__(kThreads) void k_loop_unary(LinArgs a, LoopArgs c, int n_ints, int n_lin) {
  extern __shared__ __align__(16) unsigned char s_raw[];
  __shared__ AutomatonLayout s_lay;
  loop_stage_layout(a, s_lay);
  const int g = blockIdx.y;
  LViews v(s_lay);
  double* vecs;
  if (!loop_views(a, s_lay, s_raw, n_lin, 0, n_ints, g, v, &vecs)) return;
  const LoopLin f(1. / v.zs[0]);
  const int nu = c.n_units[g];
  const int32_t* ui = c.ui + (size_t)g * c.u_stride;
  const int32_t* ud = c.ud + (size_t)g * c.u_stride;
  double* cols = c.cols + (size_t)g * c.u_stride * LOOP_COLS;
  for (int u = blockIdx.x * kThreads + threadIdx.x; u < nu; u += gridDim.x * kThreads) {
    const int i = ui[u], d = ud[u];
    cols[(size_t)LOOP_COLS * u + LC_H] = loop_hairpin(f, v.m, v.q, v.in, v.out, i, d);
    cols[(size_t)LOOP_COLS * u + LC_S] = loop_stack(f, v.m, v.q, v.in, v.out, i, d);
    cols[(size_t)LOOP_COLS * u + LC_M] = loop_multi(f, v.m, v.q, v.in, v.out, i, d);
  }
}

// grid (nb, G): the waves of the nb workgroups of slot g stride over its units
__global__ __launch_bounds__(kThreads) void k_loop_items(LinArgs a, LoopArgs c, int n_ints, int n_lin) {
  extern __shared__ __align__(16) unsigned char s_raw[];
  __shared__ AutomatonLayout s_lay;
  loop_stage_layout(a, s_lay);
  const int g = blockIdx.y;
  LViews v(s_lay);
  double* vecs;
  if (!loop_views(a, s_lay, s_raw, n_lin, kLoopWaves, n_ints, g, v, &vecs)) return;
  const int S = s_lay.S;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int lane = (int)(threadIdx.x & 63);
  double* oe = vecs + (size_t)wave * S;
  const LoopLin f(1. / v.zs[0]);
  const SeqView& q = v.q;
  const int nu = c.n_units[g];
  const int32_t* ui = c.ui + (size_t)g * c.u_stride;
  const int32_t* ud = c.ud + (size_t)g * c.u_stride;
  double* cols = c.cols + (size_t)g * c.u_stride * LOOP_COLS;
  double* T = c.T + (size_t)g * c.t_stride;
  for (int u = blockIdx.x * kLoopWaves + wave; u < nu; u += gridDim.x * kLoopWaves) {
    const int ie = ui[u] + 1, de = ud[u] - 2;
    const int oc = q.cell(ie, de);
    const int c0 = q.by_outer_off[oc], c1 = q.by_outer_off[oc + 1];
    double b = 0., n = 0.;
    if (c1 > c0) {   // (uniform over the wave: it depends on the unit alone)
      for (int s = lane; s < S; s += 64) oe[s] = f.ld(v.out, ST_E, de, ie, s);
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      for (int it = c0 + lane; it < c1; it += 64) {
        if (!loop_item_live(q, it)) continue;
        const LoopItem x = q.items[it];
        const double t = loop_two(f, v.m, q, v.in, [&](int s) { return oe[s]; }, ie, de, x);
        T[it] = t;
        if (loop_item_bulge(x)) b += t; else n += t;
      }
      for (int off = 32; off > 0; off >>= 1) {
        b += __shfl_down(b, off, 64);
        n += __shfl_down(n, off, 64);
      }
      __builtin_amdgcn_wave_barrier();   // (the next unit's out(E) overwrites the slice)
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    }
    if (lane == 0) {
      cols[(size_t)LOOP_COLS * u + LC_B] = ctx_clamp(b);
      cols[(size_t)LOOP_COLS * u + LC_I] = ctx_clamp(n);
    }
  }
}

// grid (nb, G): the lanes of the nb workgroups of slot g stride over the loops of the structure of its sequence
__global__ __launch_bounds__(kThreads) void k_loop_struct(LinArgs a, LoopArgs c, int n_ints, int n_lin) {
  extern __shared__ __align__(16) unsigned char s_raw[];
  __shared__ AutomatonLayout s_lay;
  loop_stage_layout(a, s_lay);
  const int g = blockIdx.y;
  LViews v(s_lay);
  double* vecs;
  if (!loop_views(a, s_lay, s_raw, n_lin, 0, n_ints, g, v, &vecs)) return;
  const LoopLin f(1. / v.zs[0]);
  const int64_t s0 = c.soff[v.n], s1 = c.soff[v.n + 1];
  for (int64_t t = s0 + blockIdx.x * kThreads + threadIdx.x; t < s1; t += (int64_t)gridDim.x * kThreads)
    c.s_p[t] = loop_of_structure(f, v.m, v.q, v.in, v.out, c.s_type[t], c.s_i[t], c.s_d[t], c.s_k[t], c.s_l[t]);
}

// grid (G): the counts and the list entries of the sequence idx[g], units in tiles of kThreads lanes
__global__ __launch_bounds__(kThreads) void k_loop_seq(LoopArgs c) {
  __shared__ int64_t s_scan[kThreads];
  __shared__ double s_sum[kThreads];
  const int g = blockIdx.x, tid = threadIdx.x;
  const int n = c.idx[g];
  if (c.skip_flagged && c.seq_out[(size_t)n * c.out_stride + 4] != 0.) return;
  const SeqPlan p = c.plans[n];
  const int W = p.W;
  const int nu = c.no_rss ? 0 : c.n_units[g];   // (no secondary structure in the model: no unit was written, nothing is read)
  const uint32_t* ok = c.okbits + p.bits_base;
  const double* P = c.P + (size_t)g * c.p_stride;
  const int32_t* ui = c.ui + (size_t)g * c.u_stride;
  const int32_t* ud = c.ud + (size_t)g * c.u_stride;
  const double* cols = c.cols + (size_t)g * c.u_stride * LOOP_COLS;
  const double* T = c.T + (size_t)g * c.t_stride;
  // a unit of the log-space form is any cell of the band: it counts where it is a kept cell whose P reaches the bound
  auto walked = [&](int r) {
    const int i = ui[r], d = ud[r];
    return d >= 2 && i + d <= p.L && pair_kept(ok, i, d, W) && P[(size_t)i * (W + 1) + d] >= c.bound;
  };
  if (c.counts) {
    double acc[LOOP_COLS] = {0., 0., 0., 0., 0.};
    for (int r = tid; r < nu; r += kThreads)
      if (walked(r))
        for (int k = 0; k < LOOP_COLS; ++k) acc[k] += cols[(size_t)LOOP_COLS * r + k];
    for (int k = 0; k < LOOP_COLS; ++k) {
      s_sum[tid] = acc[k];
      __syncthreads();
      for (int off = kThreads / 2; off > 0; off >>= 1) {
        if (tid < off) s_sum[tid] += s_sum[tid + off];
        __syncthreads();
      }
      if (tid == 0) c.counts[(size_t)LOOP_COLS * n + k] = s_sum[0];
      __syncthreads();
    }
  }
  if (!c.st_i) return;
  const LoopItem* items = c.items + p.item_base;
  const uint8_t* item_in = c.item_in + p.item_base;
  const int32_t* by_outer = c.by_outer_off + p.off_base;
  auto listed_item = [&](int it) {
    if (!item_in[it]) return false;
    const LoopItem x = items[it];
    return pair_kept(ok, x.k, x.l - x.k, W) && T[it] >= c.min_prob;
  };
  const int64_t k0 = c.koff[n], k2 = p.item_base;
  int64_t base = 0, base2 = 0;
  for (int r0 = 0; r0 < nu; r0 += kThreads) {
    const int r = r0 + tid;
    const bool w = r < nu && walked(r);
    const int i = w ? ui[r] : 0, d = w ? ud[r] : 2;
    const double pv = w ? P[(size_t)i * (W + 1) + d] : 0.;
    const int oc = (i + 1) * (W + 1) + (d - 2);
    const int c0 = w ? by_outer[oc] : 0, c1 = w ? by_outer[oc + 1] : 0;
    const int64_t m = w && pv >= c.min_prob ? 1 : 0;
    int64_t m2 = 0;
    for (int it = c0; it < c1; ++it)
      if (listed_item(it)) ++m2;
    int64_t total, total2;
    int64_t at = k0 + base + block_exclusive(m, s_scan, &total);
    int64_t at2 = k2 + base2 + block_exclusive(m2, s_scan, &total2);
    if (m) {
      c.st_i[at] = i; c.st_j[at] = i + d;
      c.st_v[6 * at] = pv;
      for (int k = 0; k < LOOP_COLS; ++k) c.st_v[6 * at + 1 + k] = cols[(size_t)LOOP_COLS * r + k];
    }
    for (int it = c0; it < c1; ++it)
      if (listed_item(it)) { c.st2_it[at2] = it; c.st2_t[at2] = T[it]; ++at2; }
    base += total; base2 += total2;
  }
  if (tid == 0) { c.cnt[n] = base; c.cnt2[n] = base2; }
}

// grid (n): the staging ranges of batch index blockIdx.x into their places in the two batch lists
__global__ __launch_bounds__(kThreads) void k_loop_scatter(LoopListCols c) {
  const int n = blockIdx.x;
  const SeqPlan p = c.plans[n];
  {
    const int64_t m = c.cnt[n], src = c.koff[n], dst = c.off[n];
    for (int64_t t = threadIdx.x; t < m; t += kThreads) {
      c.c_seq[dst + t] = n; c.c_i[dst + t] = c.st_i[src + t]; c.c_j[dst + t] = c.st_j[src + t];
      for (int k = 0; k < 6; ++k) c.c_v[6 * (dst + t) + k] = c.st_v[6 * (src + t) + k];
    }
  }
  const int64_t m = c.cnt2[n], src = p.item_base, dst = c.off2[n];
  for (int64_t t = threadIdx.x; t < m; t += kThreads) {
    const LoopItem x = c.items[p.item_base + c.st2_it[src + t]];
    c.t_seq[dst + t] = n; c.t_i[dst + t] = x.i - 1; c.t_j[dst + t] = x.j + 1; c.t_k[dst + t] = x.k; c.t_l[dst + t] = x.l;
    c.t_p[dst + t] = c.st2_t[src + t];
  }
}

namespace {
constexpr size_t kLdsMax = 60 * 1024;   // (with the static part below the 64 KiB a workgroup may ask for)
// the dynamic LDS of a kernel with n_vec state vectors; the blob stays in global memory where it does not fit
bool loop_lds(const LinArgs& a, int n_vec, int* n_lin, int* n_ints, size_t* lds) {
  *n_lin = kLinEth + a.lay.n_theta;   // (tau, the per-base scales, exp(theta): what lw_pair reads)
  *n_ints = a.lay.n_small;
  if (loop_lds_bytes(*n_lin, a.lay.S, n_vec, *n_ints) > kLdsMax) *n_ints = 0;
  *lds = loop_lds_bytes(*n_lin, a.lay.S, n_vec, *n_ints);
  return *lds <= kLdsMax;
}
}  // namespace

hipError_t launch_loop_unary(const LinArgs& a, const LoopArgs& c, int G, int cells_max, hipStream_t st) {
  if (G <= 0 || cells_max <= 0) return hipSuccess;
  int n_lin, n_ints; size_t lds;
  if (!loop_lds(a, 0, &n_lin, &n_ints, &lds)) return hipErrorInvalidValue;
  // (the units of a sequence are a part of its cells; a sequence's workgroups stride over them)
  const int nb = std::max(1, std::min(8, (cells_max + 4 * kThreads - 1) / (4 * kThreads)));
  hipLaunchKernelGGL(k_loop_unary, dim3(nb, G), dim3(kThreads), lds, st, lin_in_world(a), c, n_ints, n_lin);
  return hipGetLastError();
}
hipError_t launch_loop_items(const LinArgs& a, const LoopArgs& c, int G, int cells_max, hipStream_t st) {
  if (G <= 0 || cells_max <= 0) return hipSuccess;
  int n_lin, n_ints; size_t lds;
  if (!loop_lds(a, kLoopWaves, &n_lin, &n_ints, &lds)) return hipErrorInvalidValue;
  const int nb = std::max(1, std::min(16, (cells_max + 64 * kLoopWaves - 1) / (64 * kLoopWaves)));
  hipLaunchKernelGGL(k_loop_items, dim3(nb, G), dim3(kThreads), lds, st, lin_in_world(a), c, n_ints, n_lin);
  return hipGetLastError();
}
hipError_t launch_loop_struct(const LinArgs& a, const LoopArgs& c, int G, int Lmax, hipStream_t st) {
  if (G <= 0 || !c.soff) return hipSuccess;
  int n_lin, n_ints; size_t lds;
  if (!loop_lds(a, 0, &n_lin, &n_ints, &lds)) return hipErrorInvalidValue;
  const int nb = std::max(1, (Lmax / 2 + kThreads - 1) / kThreads);   // (a structure of L bases holds at most L / 2 pairs)
  hipLaunchKernelGGL(k_loop_struct, dim3(nb, G), dim3(kThreads), lds, st, lin_in_world(a), c, n_ints, n_lin);
  return hipGetLastError();
}
hipError_t launch_loop_seq(const LoopArgs& c, int G, hipStream_t st) {
  if (G <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_loop_seq, dim3(G), dim3(kThreads), 0, st, c);
  return hipGetLastError();
}
hipError_t launch_loop_scatter(const LoopListCols& c, int n, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_loop_scatter, dim3(n), dim3(kThreads), 0, st, c);
  return hipGetLastError();
}

}  // namespace elemdp
