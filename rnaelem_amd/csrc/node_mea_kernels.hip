// node_mea_kernels.hip -- maximum expected accuracy motif alignments and site lists (rule in node_mea_rules.h).
// k_node_mea runs once per call behind the node pass, over the whole-batch profile both forms of it have written: one wave per
// sequence, the lanes over the nodes (node m on lane m mod 64: one round for up to 64 nodes), the positions in order.  V(p-1, .)
// and V(p, .) lie in two LDS rows, one barrier of the single wave per position; the predecessor of every (position, node) goes to
// a scratch of M bytes per position.  The K decodes of a sequence run one after the other on the same rows and scratch, the
// earlier sites held as intervals in LDS; lane 0 walks the backpointers and writes the row and the site.  No atomics.
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "node_mea_rules.h"

namespace elemdp {

constexpr int kMeaLanes = 64;   // one wave per sequence
constexpr int kMeaNodes = 256;  // LDS row: kNodeMeaMaxNodes rounded up

// grid (n_seq)
__global__ __launch_bounds__(kMeaLanes) void k_node_mea(NodeMeaArgs a) {
  __shared__ double s_v[2][kMeaNodes];
  __shared__ int32_t s_lists[3 * kMeaNodes];
  __shared__ int32_t s_s0[kNodeMeaMaxSites], s_s1[kNodeMeaMaxSites];
  const int n = blockIdx.x, lane = threadIdx.x;
  const int M = a.M, K = a.max_sites;
  const SeqPlan pl = a.plans[n];
  const int L = pl.L;
  const size_t b = (size_t)pl.seq_base;
  for (int t = lane; t < 3 * M; t += kMeaLanes) s_lists[t] = a.lists[t];
  __syncthreads();
  const NodeMeaLists nl{s_lists, M};
  const double* prof = a.profile + (size_t)M * b;
  uint8_t* bp = a.bp + (size_t)M * b;
  uint8_t* rows = a.node + (size_t)K * b;
  const double gamma = a.gamma;
  int found = 0;
  bool done = L <= 0;
  for (int k = 0; k < K; ++k) {
    if (!done) {
      {
        const bool barred = node_mea_barred(s_s0, s_s1, found, 0);
        for (int m = lane; m < M; m += kMeaLanes) s_v[0][m] = node_mea_first(nl, gamma, prof, m, barred);
      }
      __syncthreads();
      for (int p = 1; p < L; ++p) {
        const int cur = p & 1;
        const bool barred = node_mea_barred(s_s0, s_s1, found, p);
        const double* row = prof + (size_t)M * p;
        for (int m = lane; m < M; m += kMeaLanes) {
          int from;
          s_v[cur][m] = node_mea_step(nl, gamma, row, s_v[cur ^ 1], m, barred, &from);
          bp[(size_t)M * p + m] = (uint8_t)from;
        }
        __syncthreads();   // (V(p, .) and, through the workgroup fence, the backpointers of p for lane 0)
      }
      double score;
      const int fin = node_mea_final(nl, s_v[(L - 1) & 1], &score);
      if (fin == 0) {
        done = true;   // (the best row left is all 'z': the list ends here)
      } else {
        if (lane == 0) {
          const NodeMeaSite s = node_mea_trace(nl, L, prof, bp, fin, score, rows + (size_t)k * L);
          const size_t o = (size_t)n * K + k;
          a.start[o] = s.start; a.end[o] = s.end; a.score[o] = s.score; a.conf[o] = s.conf;
          s_s0[found] = s.start; s_s1[found] = s.end;
        }
        ++found;
        __syncthreads();   // (the walk is over before the next decode overwrites the rows and the backpointers)
      }
    }
    if (done) {
      for (int p = lane; p < L; p += kMeaLanes) rows[(size_t)k * L + p] = 0;
      if (lane == 0) {
        const NodeMeaSite s = node_mea_no_site();
        const size_t o = (size_t)n * K + k;
        a.start[o] = s.start; a.end[o] = s.end; a.score[o] = s.score; a.conf[o] = s.conf;
      }
    }
  }
  if (lane == 0) a.n_sites[n] = found;
}

hipError_t launch_node_mea(const NodeMeaArgs& a, int n_seq, hipStream_t st) {
  if (n_seq <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_node_mea, dim3(n_seq), dim3(kMeaLanes), 0, st, a);
  return hipGetLastError();
}

}  // namespace elemdp
