// node_kernels.hip -- posterior motif-node profiles under the motif model (rule in node_rules.h).  k_node_pos runs on
// the compact tables of the scan's first sum pass (launch_lin_scan_group, SCAN_PASS_START), right behind it on the same slots and
// stream, before the next group of the stream reuses them.  One wave per (sequence, position): the position's result is a gather
// over the cells whose right base it is and the cells whose left base it is; lane l takes the cells of span d = 1 + l, 65 + l, ..
// of both lines, walks the transitions that emit the node (uniform lists: NodeLists), and the wave reduces with the fixed tree of
// wave_sum; lane 0 adds rule 8 and stores N(p, node).  No per-cell scratch, no atomics: repeats over the same tables give the same
// bits.  A sequence the range check flagged is left to the log-space form (the fused scan kernel, DpArgs::node).
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "lin_views.h"
#include "node_rules.h"
#include "wave_gather.h"

namespace elemdp {

constexpr int kNodeWaves = kThreads / 64;   // positions per workgroup

// grid (ceil(L / kNodeWaves), G)
__global__ __launch_bounds__(kThreads) void k_node_pos(LinArgs a, NodeArgs c) {
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
  const int p = __builtin_amdgcn_readfirstlane(blockIdx.x * kNodeWaves + (int)(threadIdx.x >> 6));
  if (p >= L) return;
  const int lane = threadIdx.x & 63;
  const NodeLin f(1. / v.zs[0]);
  const NodeLists nl{c.lists, c.M, c.rules};
  double* row = c.profile + (size_t)c.M * (size_t)(v.seq_base + p);
  for (int node = 0; node < c.M; ++node) {
    const double cells = wave_sum(c.no_rss ? 0. : node_cells_part(f, nl, v.m, v.q, v.in, v.out, p, node, lane, 64));
    if (lane == 0) row[node] = node_finish(cells, node_exterior(f, nl, v.m, v.q, v.in, v.out, p, node));
  }
}

hipError_t launch_node_pos(const LinArgs& a, const NodeArgs& c, int G, int Lmax, hipStream_t st) {
  if (G <= 0 || Lmax <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_node_pos, dim3((Lmax + kNodeWaves - 1) / kNodeWaves, G), dim3(kThreads), 0, st, lin_in_world(a), c);
  return hipGetLastError();
}

}  // namespace elemdp
