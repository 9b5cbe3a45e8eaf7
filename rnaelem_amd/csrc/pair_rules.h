// pair_rules.h -- base-pair posteriors under the motif model, host / device.
//
//   P(i, j = i + d) = sum over the real interval states s of inside(i, j, ST_P, s) * outside(i, j, ST_P, s) / Z(ari, nasi)
//
// over the tables of the scan's first sum pass (terminals ari and nasi).  Bases i and j-1 (0-based) pair.  A cell the BPP filter
// did not keep has P = 0 and its table entries are never read.  The scaled-linear tables need no rescaling: every parse emits
// every position once, so inside x outside carries the scale of the whole sequence, as Z does.  One rule for both forms: the
// compact scaled-linear rows of pair_kernels.hip (PairLin) and the dense log-space rows of the fused scan kernel (PairLog).
#pragma once
#include "dp_rules.h"

namespace elemdp {

ELEMDP_HD bool pair_kept(const uint32_t* okbits, int i, int d, int W) {
  const uint32_t c = (uint32_t)i * (uint32_t)(W + 1) + (uint32_t)d;
  return ((okbits[c >> 5] >> (c & 31)) & 1u) != 0;
}

// terms of one state, summed by the caller in increasing column / state order, then finished once per cell
struct PairLin {
  double invZ;   // 1 / the mantissa of Z(ari, nasi) in the tables' scale
  ELEMDP_HD double term(double in, double out) const { return in * out; }
  ELEMDP_HD double finish(double acc) const { return acc * invZ; }
};
struct PairLog {
  double lnZ;
  ELEMDP_HD double term(double in, double out) const { return exp(in + out - lnZ); }
  ELEMDP_HD double finish(double acc) const { return acc; }
};

// unpaired(p) = 1 - sum_d P(p, d) - sum_i P(i, p+1-i): first the pairs whose left base is p in increasing d, then those whose
// right base is p in increasing i.  P: one sequence's [i][d] array (rows of W+1), 0 where the cell is not kept.
ELEMDP_HD double pair_unpaired(const double* P, const uint32_t* okbits, int L, int W, int p) {
  double left = 0., right = 0.;
  for (int d = 1; d <= W && p + d <= L; ++d)
    if (pair_kept(okbits, p, d, W)) left += P[(size_t)p * (W + 1) + d];
  for (int i = p + 1 - W < 0 ? 0 : p + 1 - W; i <= p; ++i)
    if (pair_kept(okbits, i, p + 1 - i, W)) right += P[(size_t)i * (W + 1) + (p + 1 - i)];
  return 1. - left - right;
}

}  // namespace elemdp
