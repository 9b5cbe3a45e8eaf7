// cond_rules.h -- motif-conditional pair posteriors, host / device.
//
// The ensemble of the scan's first sum pass is a mixture of two worlds: the parses with the motif (terminals ari) and those
// without it (terminal nasi), Z(ari, nasi) = Z(ari) + Z(nasi).  Outside values are linear in the terminal vector, so an outside
// sweep seeded with one world's terminals alone gives that world's outside tables over the same inside tables, and
//
//   P_motif(i, j) = sum_s inside(i, j, ST_P, s) * outside_ari (i, j, ST_P, s) / Z(ari)
//   P_none (i, j) = sum_s inside(i, j, ST_P, s) * outside_nasi(i, j, ST_P, s) / Z(nasi)
//
// are the pair rule of pair_rules.h (PairLin / PairLog, the real interval states in column order) with the world's own Z.  Per
// world, unpaired(p) is pair_unpaired over that world's P.  Over both,
//
//   exist_prob = Z(ari) / Z(ari, nasi)
//   shift      = sum over the kept cells, in (i, d) order, of |P_motif - P_none|
//
// A world with Z = 0 is empty: P = 0, unpaired = 1, shift = NaN, and exist_prob is 0 (no parse with the motif, or none at all)
// or 1 (none without it).
#pragma once
#include "pair_rules.h"

namespace elemdp {

enum CondWorld : int { COND_MOTIF = 0, COND_NONE = 1 };

// the three partition functions of a sequence as the tables carry them: mantissas in the tables' scale (scaled-linear form) or
// logarithms (log-space form)
struct CondZ {
  double zo, za, zn;
  bool log;
  ELEMDP_HD double of(int world) const { return world == COND_MOTIF ? za : zn; }
  ELEMDP_HD bool empty(int world) const { return log ? !(of(world) > ELEMDP_NEG_INF) : !(of(world) > 0.); }
  ELEMDP_HD double exist() const {
    if (empty(COND_MOTIF)) return 0.;
    if (empty(COND_NONE)) return 1.;
    return log ? exp(za - zo) : za / zo;
  }
};

// one row of the shift: |P_motif - P_none| over the kept cells (i, d = 1 .. dmax) in increasing d; the caller adds the rows in
// increasing i
ELEMDP_HD double cond_shift_row(const double* P0, const double* P1, const uint32_t* okbits, int W, int i, int dmax) {
  double acc = 0.;
  for (int d = 1; d <= dmax; ++d)
    if (pair_kept(okbits, i, d, W)) acc += fabs(P0[(size_t)i * (W + 1) + d] - P1[(size_t)i * (W + 1) + d]);
  return acc;
}

// does the list keep the cell?  (min_prob = +inf keeps none; a NaN never arises: P is a finite sum or an exact 0)
ELEMDP_HD bool cond_listed(double p0, double p1, double min_prob) { return (p0 > p1 ? p0 : p1) >= min_prob; }

}  // namespace elemdp
