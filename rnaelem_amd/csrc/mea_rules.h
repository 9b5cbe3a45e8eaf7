// mea_rules.h -- maximum expected accuracy structures under the motif model, host / device.
//
// Over the pair posteriors P(i, e) of pair_rules.h (bases i and i+e-1 pair; only kept cells) and q(p) = unpaired(p), with
// w(i, e) = RN(2 gamma * P(i, e)), the structure maximises the sum of w over its pairs plus the sum of q over its unpaired bases
// (Do et al. 2006; ViennaRNA's MEA).  Banded table M(i, d) = the best score of bases [i, i+d), d <= W, M(i, 0) = 0:
//
//   M(i, d) = max( M(i+1, d-1) + q(i),  over kept (i, e), e = 2 .. d:  (w(i, e) + M(i+1, e-2)) + M(i+e, d-e) )
//
// and the exterior chain F(i) = the best score of [i, L), F(L) = 0, with F(i+1) and F(i+e) in place of M(i+1, d-1) and
// M(i+e, d-e), e = 2 .. min(W, L-i).  Score = F(0).  Candidates are taken in the order written (unpaired first, then e
// increasing) and a later one replaces the current one only if it is strictly greater, as `compare` does in the scan: the
// traceback follows exactly the argmax of the forward pass, and the sums are added in exactly the order written (no fma).
#pragma once
#include "pair_rules.h"
#include "scan_rules.h"

namespace elemdp {

// a pair candidate: (w(i, e) + M(i+1, e-2)) + rest, rest = M(i+e, d-e) or F(i+e).  HIP's __dmul_rn is a plain product, which
// the default -ffp-contract=fast fuses with the sum behind it (one rounding instead of two, visible whenever 2 gamma P is not
// exact, e.g. gamma = 1e3): contraction is off here, so that w is rounded before any sum.
ELEMDP_HD double mea_pair(double gamma2, double p, double inner, double rest) {
#pragma clang fp contract(off)
  const double w = gamma2 * p;
  return (w + inner) + rest;
}

// the first strictly greatest of two partial maxima of one candidate list, e = their first candidates (0 = none)
ELEMDP_HD void mea_merge(double& best, int& e, double other, int other_e) {
  if (other > best || (other == best && other_e != 0 && (e == 0 || other_e < e))) { best = other; e = other_e; }
}

// M(i, d) of one sequence in candidate order; P and M: [i][d] arrays with rows of W+1, q: unpaired.  Visits only the kept
// cells of row i, a mask word at a time.  Returns the choice: 0 = base i unpaired, else e.
ELEMDP_HD int mea_band_cell(const double* P, const double* M, const double* q, const uint32_t* okbits, int W, double gamma2, int i,
                            int d, double* out) {
  const size_t R = (size_t)(W + 1);
  double best = M[(size_t)(i + 1) * R + (d - 1)] + q[i];
  int ch = 0;
  const uint32_t c0 = (uint32_t)i * (uint32_t)(W + 1);
  for (uint32_t lo = c0 + 2, hi = c0 + (uint32_t)d; lo <= hi;) {
    const uint32_t sh = lo & 31u, nb = (32u - sh) < (hi - lo + 1u) ? (32u - sh) : (hi - lo + 1u);
    uint32_t bits = okbits[lo >> 5] >> sh;
    if (nb < 32u) bits &= (1u << nb) - 1u;
    while (bits) {
      const int e = (int)(lo - c0) + __builtin_ctz(bits);
      bits &= bits - 1u;
      const double v = mea_pair(gamma2, P[(size_t)i * R + e], M[(size_t)(i + 1) * R + (e - 2)], M[(size_t)(i + e) * R + (d - e)]);
      if (v > best) { best = v; ch = e; }
    }
    lo += nb;
  }
  *out = best;
  return ch;
}

}  // namespace elemdp
