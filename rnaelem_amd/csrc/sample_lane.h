// sample_lane.h -- one sample of one sequence into the outputs of SampleArgs (device code of k_sample and of the fused scan kernel).
#pragma once
#include "kernels.h"
#include "sample_rules.h"

namespace elemdp {

// sample k of batch index n (outputs at base = n_samples * seq_base): the walk, or blank letters, node 0 and a NaN log-probability
// when it fails; returns the walk's SampleStatus
template <class Tab>
__device__ __forceinline__ int sample_one(const ModelView& m, const SeqView& q, const Tab& T, const SampleArgs& sa, int n, int64_t base,
                                          int L, int k, TraceFrame* stack) {
  char* rss = sa.rss + base + (int64_t)k * L;
  uint8_t* node = sa.node + base + (int64_t)k * L;
  for (int p = 0; p < L; ++p) { rss[p] = ' '; node[p] = 0; }
  double lp = NAN;
  const int r = sample_walk(m, q, T, sa.seed, (uint64_t)(sa.index_base + n), (uint64_t)k, node, rss, &lp, stack, sa.stack_cap, sa.world);
  if (r != SAMPLE_OK) {
    lp = NAN;
    for (int p = 0; p < L; ++p) { rss[p] = ' '; node[p] = 0; }
  }
  sa.logp[(size_t)n * sa.n_samples + k] = lp;
  return r;
}

}  // namespace elemdp
