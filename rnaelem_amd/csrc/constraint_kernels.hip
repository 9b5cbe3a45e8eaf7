// constraint_kernels.hip -- hard structure constraints per sequence (rule in constraint_rules.h).  k_constrain turns
// the pair mask the BPP filter left (`in`, which may be the output itself) into the mask of the constrained ensemble, behind the filter and before the plan
// builder.  Grid (chunks of 256 mask words, sequences), as the plan builder's kernels; one lane owns one 32-bit word: it reads the
// filter's word, drops the cells the constraint does not allow, adds the forced pairs of the word's rows and writes the word
// with a plain store.  No atomics, and no two lanes touch one word.  The per-position rows (a byte and two ints per base) are read
// through the cache: the lanes of a wave share a few rows, and the words of a filtered mask hold few set bits.
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "constraint_rules.h"

namespace elemdp {

__global__ __launch_bounds__(kThreads) void k_constrain(const SeqPlan* plans, ConsView cons, const uint32_t* in, uint32_t* okbits) {
  const SeqPlan& p = plans[blockIdx.y];   // (four fields of it, uniform over the workgroup)
  const int L = p.L, W = p.W;
  const int ncell = (L + 1) * (W + 1), nword = (ncell + 31) / 32;
  const int w = blockIdx.x * kThreads + threadIdx.x;
  if (w >= nword) return;
  const ConsView c{cons.cls + p.pos_base, cons.partner + p.pos_base, cons.enc + p.pos_base};
  const size_t at = (size_t)p.bits_base + w;
  okbits[at] = cons_word(c, L, W, w, in[at]);
}

hipError_t launch_constrain(const SeqPlan* plans, int n_seq, int nword_max, const uint8_t* cls, const int32_t* partner,
                            const int32_t* enc, const uint32_t* in, uint32_t* okbits, hipStream_t st) {
  if (n_seq <= 0 || nword_max <= 0) return hipSuccess;
  const ConsView c{cls, partner, enc};
  hipLaunchKernelGGL(k_constrain, dim3((nword_max + kThreads - 1) / kThreads, n_seq), dim3(kThreads), 0, st, plans, c, in, okbits);
  return hipGetLastError();
}

}  // namespace elemdp
