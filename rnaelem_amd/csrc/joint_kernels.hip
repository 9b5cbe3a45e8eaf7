// joint_kernels.hip -- joint node-by-context posteriors and emission counts (rule in joint_rules.h).  k_joint_rows and
// k_joint_pos run on the compact tables of the scan's first sum pass (launch_lin_scan_group, SCAN_PASS_START), right behind it on
// the same slots and stream, before the next group of the stream reuses them.
//   k_joint_rows   one wave per row i of a sequence, d from min(W, L - i) down to 1; lane = interval state.  The vectors G_H and G_B
//                  of the step and of the step before, and the row's in(L), live in the wave's slice of LDS (any state count: the
//                  slice is sized at the launch).  Per step a lane forms the two seeds of its state and takes the chain step; then
//                  lane = node sums in(L) G_c / Z over the loop states that emit the node and stores the two sums of the cell.
//   k_joint_pos    one wave per (sequence, position), as k_node_pos: lane l takes the spans d = 1 + l, 65 + l, ..; per node the five
//                  routed parts of node_rules.h and the H and B sums along the anti-diagonal, reduced with the fixed tree of
//                  wave_sum; lane 0 adds rule 8, forms I, clamps and stores the 7 letters.
//   k_joint_counts one workgroup per sequence, one lane per (node, letter, base), positions in increasing order; it serves the
//                  log-space form too, whose profile the fused scan kernel writes (DpArgs::jnt).
// No atomics: every sum has a fixed order, so repeats over the same tables give the same bits.  A sequence the range check flagged
// is left to the log-space form.
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "lin_views.h"
#include "joint_rules.h"
#include "lin_params.h"
#include "wave_gather.h"

namespace elemdp {

constexpr int kJointWaves = kThreads / 64;   // rows (k_joint_rows) or positions (k_joint_pos) per workgroup

__device__ __forceinline__ void joint_wave_sync() {
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
}

// dynamic LDS of k_joint_rows (bytes): the linear parameter block, kJointWaves slices of 5 S doubles (in(L) of the cell, G_H and G_B
// of the step and of the step before), the small part of the automaton blob (n_ints of them, 0: left in global memory)
__host__ __device__ inline size_t joint_lds_bytes(int n_lin, int S, int n_ints) {
  return 8 * ((size_t)n_lin + (size_t)kJointWaves * 5 * (size_t)S) + 4 * (size_t)n_ints;
}

__device__ __forceinline__ JointLists joint_lists(const JointArgs& c) {
  return JointLists{NodeLists{c.lists, c.M, NR_ALL}, c.lists + c.slot_at, c.n_slots, JP_ALL};
}

// grid (ceil(L / kJointWaves), G).  The automaton blob and the linear parameter block are staged as k_access_chains stages them:
// every step of the chain reads per-state attributes, a transition list and an emission weight.
__global__ __launch_bounds__(kThreads) void k_joint_rows(LinArgs a, JointArgs c, int n_ints, int n_lin) {
  extern __shared__ __align__(16) unsigned char s_raw[];
  __shared__ AutomatonLayout s_lay;
  {
    const int32_t* src = reinterpret_cast<const int32_t*>(a.layp);
    int32_t* dst = reinterpret_cast<int32_t*>(&s_lay);
    for (int t = threadIdx.x; t < (int)(sizeof(AutomatonLayout) / sizeof(int32_t)); t += kThreads) dst[t] = src[t];
  }
  double* llin = reinterpret_cast<double*>(s_raw);
  __syncthreads();
  const int S = s_lay.S;
  double* slices = llin + n_lin;
  int32_t* blob = reinterpret_cast<int32_t*>(slices + (size_t)kJointWaves * 5 * S);
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
  const int L = v.q.L, W = v.q.W;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int i = blockIdx.x * kJointWaves + wave;
  if (i >= L) return;
  const int lane = threadIdx.x & 63;
  const JointLin f(1. / v.zs[0]);
  const JointLists jl = joint_lists(c);
  double* X = c.X + (size_t)g * c.x_stride;
  double* inL = slices + (size_t)wave * 5 * S;
  double* cur[2] = {inL + S, inL + 2 * S};
  double* prev[2] = {inL + 3 * S, inL + 4 * S};
  const int32_t* I = v.m.ints;
  const int dmax = L - i < W ? L - i : W;
  for (int d = dmax; d >= 1; --d) {
    for (int s = lane; s < S; s += 64) {
      JointG gg{0., 0.};
      double x = 0.;
      if (I[s_lay.st_is_loop + s]) {
        x = f.ld(v.in, ST_L, d, i, s);
        if (!f.dead(x)) gg = joint_entry(f, jl, v.m, v.q, v.in, v.out, d, i, s, d < dmax ? prev[0] : nullptr, d < dmax ? prev[1] : nullptr);
      }
      inL[s] = x; cur[0][s] = gg.h; cur[1][s] = gg.b;
    }
    joint_wave_sync();
    for (int node = lane; node < c.M; node += 64) {
      const int k = jl.slot[node];
      if (k < 0) continue;
      X[joint_cell_at(v.q, jl.n_slots, i, d, JK_H) + k] = joint_node_sum(f, jl.nl, node, inL, cur[0]);
      X[joint_cell_at(v.q, jl.n_slots, i, d, JK_B) + k] = joint_node_sum(f, jl.nl, node, inL, cur[1]);
    }
    joint_wave_sync();   // (the next step writes in(L) and the vectors of the step before this one)
    for (int k = 0; k < 2; ++k) { double* t = cur[k]; cur[k] = prev[k]; prev[k] = t; }
  }
}

// grid (ceil(L / kJointWaves), G)
__global__ __launch_bounds__(kThreads) void k_joint_pos(LinArgs a, JointArgs c) {
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
  const int L = v.q.L;
  const int p = __builtin_amdgcn_readfirstlane(blockIdx.x * kJointWaves + (int)(threadIdx.x >> 6));
  if (p >= L) return;
  const int lane = threadIdx.x & 63;
  const JointLin f(1. / v.zs[0]);
  const JointLists jl = joint_lists(c);
  const double* X = c.X + (size_t)g * c.x_stride;
  double* row = c.profile + (size_t)CTX_COLS * c.M * (size_t)(v.seq_base + p);
  for (int node = 0; node < c.M; ++node) {
    JointParts part{0., 0., 0., 0.};
    double h = 0., b = 0.;
    if (!c.no_rss) {
      part = joint_cells_part(f, jl.nl, v.m, v.q, v.in, v.out, p, node, lane, 64);
      part.l = wave_sum(part.l); part.r = wave_sum(part.r); part.u = wave_sum(part.u); part.mm = wave_sum(part.mm);
      const int k = jl.slot[node];
      if (k >= 0) {   // (uniform: the node alone decides)
        h = wave_sum(joint_gather_part(X, v.q, jl.n_slots, p, k, JK_H, lane, 64));
        b = wave_sum(joint_gather_part(X, v.q, jl.n_slots, p, k, JK_B, lane, 64));
      }
    }
    if (lane == 0) joint_compose(joint_exterior(f, jl.nl, v.m, v.q, v.in, v.out, p, node), part, h, b, row + CTX_COLS * node);
  }
}

// grid (G): the counts of the sequence idx[g]
__global__ __launch_bounds__(kThreads) void k_joint_counts(JointArgs c) {
  const int g = blockIdx.x;
  const int n = c.idx[g];
  if (c.skip_flagged && c.seq_out[(size_t)n * c.out_stride + 4] != 0.) return;
  const SeqPlan p = c.plans[n];
  const int nc = c.M * CTX_COLS * kJointBases;
  const double* prof = c.profile + (size_t)CTX_COLS * c.M * (size_t)p.seq_base;
  double* counts = c.counts + (size_t)nc * n;
  for (int t = threadIdx.x; t < nc; t += kThreads) counts[t] = joint_count(prof, c.seq + p.seq_base, p.L, c.M, t);
}

hipError_t launch_joint_rows(const LinArgs& a, const JointArgs& c, int G, int Lmax, hipStream_t st) {
  if (G <= 0 || Lmax <= 0) return hipSuccess;
  constexpr size_t kLdsMax = 60 * 1024;   // (with the static part below the 64 KiB a workgroup may ask for)
  const int n_lin = kLinEth + a.lay.n_theta;   // (tau, the per-base scales, exp(theta): what lw_right reads)
  int n_ints = a.lay.n_small;
  if (joint_lds_bytes(n_lin, a.lay.S, n_ints) > kLdsMax) n_ints = 0;   // (a large automaton: its blob stays in global memory)
  const size_t lds = joint_lds_bytes(n_lin, a.lay.S, n_ints);
  if (lds > kLdsMax) return hipErrorInvalidValue;   // (more than a thousand interval states: no such pattern is accepted)
  hipLaunchKernelGGL(k_joint_rows, dim3((Lmax + kJointWaves - 1) / kJointWaves, G), dim3(kThreads), lds, st, lin_in_world(a), c, n_ints, n_lin);
  return hipGetLastError();
}
hipError_t launch_joint_pos(const LinArgs& a, const JointArgs& c, int G, int Lmax, hipStream_t st) {
  if (G <= 0 || Lmax <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_joint_pos, dim3((Lmax + kJointWaves - 1) / kJointWaves, G), dim3(kThreads), 0, st, lin_in_world(a), c);
  return hipGetLastError();
}
hipError_t launch_joint_counts(const JointArgs& c, int G, hipStream_t st) {
  if (G <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_joint_counts, dim3(G), dim3(kThreads), 0, st, c);
  return hipGetLastError();
}

}  // namespace elemdp
