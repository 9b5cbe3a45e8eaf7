// sample_kernels.hip -- stochastic samples of derivations under the motif model (rule in sample_rules.h).
// k_sample runs on the inside tables of launch_lin_scan_group (SCAN_PASS_INSIDE), right behind it on the same slots and stream
// (before the next group of the stream reuses them): one wave per sequence, one lane per sample (samples k = lane, lane + 64, ..), each lane
// walking its own derivation with its stack in the slot's scratch (min(n_samples, 64) x stack_cap frames, sample_stack_cap).  A
// sequence the range check flagged is left to the fused scan kernel (DpArgs::smp).
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "lin_views.h"
#include "sample_rules.h"
#include "sample_lane.h"

namespace elemdp {

__global__ __launch_bounds__(kSampleLanes) void k_sample(LinArgs a, SampleArgs sa) {
  __shared__ AutomatonLayout s_lay;
  {
    const int32_t* src = reinterpret_cast<const int32_t*>(a.layp);
    int32_t* dst = reinterpret_cast<int32_t*>(&s_lay);
    for (int t = threadIdx.x; t < (int)(sizeof(AutomatonLayout) / sizeof(int32_t)); t += kSampleLanes) dst[t] = src[t];
  }
  __syncthreads();
  const int g = blockIdx.x, lane = threadIdx.x;
  LViews v(s_lay);
  make_lviews(a, g, v);
  const int L = v.q.L, n = v.n;
  const int64_t base = (int64_t)sa.n_samples * v.seq_base;
  if (v.row[4] != 0.) return;   // (outside the double range: the log-space form of the fused scan kernel samples it)
  TraceFrame* stack = sa.stack + ((size_t)g * sa.stack_lanes + min(lane, sa.stack_lanes - 1)) * (size_t)sa.stack_cap;
  const LinSampleTab T{v.in};
  int status = SAMPLE_OK;
  for (int k = lane; k < sa.n_samples; k += kSampleLanes)
    status = max(status, sample_one(v.m, v.q, T, sa, n, base, L, k, stack));
  for (int off = kSampleLanes / 2; off > 0; off >>= 1) status = max(status, __shfl_xor(status, off));
  if (lane == 0) sa.status[n] = status;
}

hipError_t launch_sample(const LinArgs& a, const SampleArgs& s, int G, hipStream_t st) {
  if (G <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_sample, dim3(G), dim3(kSampleLanes), 0, st, a, s);
  return hipGetLastError();
}

}  // namespace elemdp
