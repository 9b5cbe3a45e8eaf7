// block_scan.h -- the workgroup prefix sum of the list kernels (pair_kernels.hip, stem_kernels.hip), device code.
#pragma once
#include <hip/hip_runtime.h>

#include "kernels.h"

namespace elemdp {

// exclusive prefix over the workgroup (kThreads lanes); returns the workgroup's total through *total
__device__ inline int64_t block_exclusive(int64_t v, int64_t* s, int64_t* total) {
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

}  // namespace elemdp
