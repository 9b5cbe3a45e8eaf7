// plan_rules.h -- parameter-independent per-sequence preparation ("plan"), host/device agnostic.
//
// Everything the reference recomputes inside its sweep on every optimizer step although it does
// not depend on theta / lambda is computed once per batch and kept resident in HBM:
//   * which cells may hold a base pair      EnergyModel::fill_bpp_tables  energy_model.hpp:211-266
//   * the structural term of every rule     the tsc arguments at          energy_model.hpp:346-437
//   * the interior-loop candidates (k,l)    the double loop at            energy_model.hpp:413-426
//     (inside enumeration) and :527-541 (outside enumeration, a superset when C < 30)
#pragma once
#include "dp_rules.h"
#include "energy_rules.h"
#include "live_blocks.h"

namespace elemdp {

struct PlanCfg {
  int32_t no_ene;    // --no-energy: every structural term is 0 (energy_model.hpp:351,372,399,...)
  int32_t min_span;  // smallest span of a base-pair cell: turn+2 = 5, or 1 with NO_TURN (:217)
  int32_t fix_rss;   // structure given per sequence
};

// ndot[p] = number of non-'.' characters in fix[0..p); segment [a,b) is all dots iff equal counts
ELEMDP_HD bool all_dots(const int32_t* ndot, int a, int b) { return ndot == nullptr || ndot[b] == ndot[a]; }

// canonical candidate: cell (i,d) may pair by sequence alone (energy_model.hpp:216-219)   (host too: the check of a forced pair)
ELEMDP_HOSTDEV bool canonical_pair(const uint8_t* seq, int L, int W, int min_span, int i, int d) {
  return d >= min_span && d <= W && i + d <= L && bp_type(seq[i], seq[i + d - 1]) > 0;
}

struct PairTerms { double stack, ext, ml, close, hp; };

// structural terms of a kept pair cell (i,d); `inner_ok` = cell (i+1,d-2) is kept too
ELEMDP_HD PairTerms pair_terms(const EnergyTables& e, const PlanCfg& cfg, const uint8_t* seq, int L, const int32_t* ndot,
                               int i, int d, bool inner_ok) {
  const int j = i + d;
  PairTerms t;
  const double NEG = ELEMDP_NEG_INF;
  t.stack = inner_ok ? (cfg.no_ene ? 0. : loop_energy(e, seq, i, j - 1, i + 1, j - 2)) : NEG;     // :351-352
  t.ext = cfg.no_ene ? 0. : sum_ext_m(e, seq, L, i, j - 1, true);                                  // :429-430
  t.ml = cfg.no_ene ? 0. : sum_ext_m(e, seq, L, i, j - 1, false) + e.ml_intern;                    // :372-373
  t.close = cfg.no_ene ? 0. : sum_ext_m(e, seq, L, j - 1, i, false) + (e.ml_closing + e.ml_intern);  // :399-402
  t.hp = cfg.no_ene ? 0. : hairpin_energy(e, seq, i, j - 1);                                       // :407-408
  if (!all_dots(ndot, i + 1, j - 1)) t.hp = NEG;                                                   // :409-410
  return t;
}

// Enumerates the interior-loop candidates of the E cell (i,d) (closing pair = cell (i-1,d+2)) in the
// reference's inside order (l descending, k ascending) over the OUTSIDE set
//   i <= k <= min(j-2, i+C),  k+2 <= l <= j,  (k,l) != (i,j),  P(k,l) kept,  tsc finite
// and calls f(k, l, tsc, in_inside_set) for each; in_inside_set <=> (k-i)+(j-l) <= C.
template <class OkFn, class F>
ELEMDP_HD void enum_interior(const EnergyTables& e, const PlanCfg& cfg, const uint8_t* seq, int L, int W, int C,
                             const int32_t* ndot, const OkFn& ok, int i, int d, F&& f) {
  const int j = i + d;
  for (int l = j; l >= i + 2; --l) {
    const int kmax = (l - 2 < i + C) ? l - 2 : i + C;
    for (int k = i; k <= kmax; ++k) {
      if (k == i && l == j) continue;
      if (l - k > W || !ok(k, l - k)) continue;
      const double tsc = cfg.no_ene ? 0. : loop_energy(e, seq, i - 1, j, k, l - 1);
      if (tsc == ELEMDP_NEG_INF) continue;
      if (!all_dots(ndot, i, k) || !all_dots(ndot, l, j)) continue;  // :419-421
      f(k, l, tsc, (k - i) + (j - l) <= C);
    }
  }
}

// The same enumeration, in the same order, from the END-major pair mask (bit l * (W+1) + (l - k) <=> pair cell (k, l-k)):
// for a fixed end l the candidates k = i .. kmax are one run of bits (k ascending = span descending), so only kept pairs
// are visited -- ~(d-1) short bit runs per E cell instead of up to C * d single tests.  `word(n)` returns the n-th 32-bit
// word of the mask (0 past the end).
template <class WordFn, class F>
ELEMDP_HD void enum_interior_by_end(const EnergyTables& e, const PlanCfg& cfg, const uint8_t* seq, int L, int W, int C,
                                    const int32_t* ndot, const WordFn& word, int i, int d, F&& f) {
  const int j = i + d;
  for (int l = j; l >= i + 2; --l) {
    const int kmax = (l - 2 < i + C) ? l - 2 : i + C;
    const int dhi = (l - i < W) ? l - i : W, dlo = l - kmax;   // spans l - k of the candidates k = i .. kmax
    for (int top = dhi; top >= dlo; top -= 32) {
      const int lo = (top - 31 > dlo) ? top - 31 : dlo;
      const int len = top - lo + 1;
      const long long b0 = (long long)l * (W + 1) + lo;
      const int w = (int)(b0 >> 5), sh = (int)(b0 & 31);
      const unsigned long long two = ((unsigned long long)word(w + 1) << 32) | (unsigned long long)word(w);
      uint32_t m = (uint32_t)(two >> sh);
      if (len < 32) m &= (1u << len) - 1u;
      while (m) {
        const int b = 31 - __builtin_clz(m);
        m &= ~(1u << b);
        const int k = l - (lo + b);
        if (k == i && l == j) continue;
        const double tsc = cfg.no_ene ? 0. : loop_energy(e, seq, i - 1, j, k, l - 1);
        if (tsc == ELEMDP_NEG_INF) continue;
        if (!all_dots(ndot, i, k) || !all_dots(ndot, l, j)) continue;
        f(k, l, tsc, (k - i) + (j - l) <= C);
      }
    }
  }
}

// The NUMBER of candidates enum_interior_by_end visits, from popcounts of the same bit runs -- valid when no loop term is log 0
// except by size (loop_tables_finite, energy_tables.h; a sequence without N) and no structure is imposed (ndot == nullptr): then a kept pair (k, l) is
// dropped only where the loop would hold more than kMaxLoop unpaired bases (loop_energy, energy_rules.h:77).  The count pass of
// the plan builder (k_plan_cells) evaluated the energy of every candidate just to test it against log 0.
template <class WordFn>
ELEMDP_HD int count_interior_by_end(bool no_ene, int L, int W, int C, const WordFn& word, int i, int d) {
  const int j = i + d;
  int n = 0;
  for (int l = j; l >= i + 2; --l) {
    int kmax = (l - 2 < i + C) ? l - 2 : i + C;
    if (!no_ene) {
      const int kcap = i + kMaxLoop - (j - l);
      if (kcap < kmax) kmax = kcap;
      if (kmax < i) break;            // (the right side alone exceeds kMaxLoop from here on)
    }
    const int dhi = (l - i < W) ? l - i : W, dlo = l - kmax;
    for (int top = dhi; top >= dlo; top -= 32) {
      const int lo = (top - 31 > dlo) ? top - 31 : dlo;
      const int len = top - lo + 1;
      const long long b0 = (long long)l * (W + 1) + lo;
      const int w = (int)(b0 >> 5), sh = (int)(b0 & 31);
      const unsigned long long two = ((unsigned long long)word(w + 1) << 32) | (unsigned long long)word(w);
      uint32_t m = (uint32_t)(two >> sh);
      if (len < 32) m &= (1u << len) - 1u;
      n += __builtin_popcount(m);
    }
  }
  if (d <= W && d >= 2) {             // (k, l) = (i, j): the closing pair's stack (rule 1b), not a loop
    const long long b = (long long)j * (W + 1) + d;
    if ((word((int)(b >> 5)) >> (b & 31)) & 1u) --n;
  }
  return n;
}

// ---------------------------------------------------------------------------------------------
// Usefulness mask: one byte per band cell, [d][i] like the tables.  Bit (cell, plane) is set when a complete parse
// can pass through that entry in the structure grammar with every weight taken as positive; an entry whose bit is clear has
// inside value 0 or outside value 0 for every theta / lambda.  The mask may be a superset of that set, never miss an entry.
// Two boolean sweeps with the conditions the band kernels test (lin_fast.h: cell_in_flags / cell_out_flags, the pair phases of
// k4_in / k4_out): inside liveness bottom-up (useful_inside_cell: reads rows of smaller span), then outside reachability
// top-down through the inside-live entries only (useful_outside_cell: reads rows of larger span, and the cell's own inside
// bits, which it replaces -- the sweep works in place).  All cells of one diagonal are independent in either sweep.
// ---------------------------------------------------------------------------------------------
// (these run on the host too -- the host entry of the C ABI -- where the recurrences of dp_rules.h are device code only)
enum : int { UB_P = 1, UB_E = 2, UB_M = 4, UB_B = 8, UB_A = 16, UB_1 = 32, UB_2 = 64, UB_L = 128, UB_ALL = 255 };
static_assert(kLiveInsideBits == (UB_ALL & ~UB_L), "live_blocks.h: the bits of the inside lists behind the loop pre-pass");

struct UsefulCtx {
  int32_t L, W, C, m_min;
  int32_t loop_cap;          // an interior loop holds at most this many unpaired bases (kMaxLoop; no bound under --no-energy)
  const uint32_t* okbits;    // kept pairs, bit i * (W+1) + d (one word of slack behind the last: the bit walks read ahead)
  const uint32_t* okbits_end;   // the same pairs by (end, span): bit j * (W+1) + d <=> pair cell (j - d, d)  (k_mask_by_end)
  const int16_t* dmin;       // L+1
  const uint8_t* unp;        // L
  ELEMDP_HOSTDEV bool pair_ok(int i, int d) const {
    if (i < 0 || d < 0 || d > W || i + d > L) return false;
    const int c = i * (W + 1) + d;
    return (okbits[c >> 5] >> (c & 31)) & 1u;
  }
  ELEMDP_HOSTDEV bool left_ok(int i, int d) const {
    if (d > W || d < 0 || i + d > L) return false;
    const int dm = dmin[i];
    return dm > 0 && d >= dm;
  }
  ELEMDP_HOSTDEV bool e_ok(int i, int d) const { return i > 0 && d + 2 <= W && pair_ok(i - 1, d + 2); }
  ELEMDP_HOSTDEV bool m_ok(int i, int d) const { return 0 < i && i + d < L && d <= W && m_min <= d; }
  ELEMDP_HOSTDEV int at(int i, int d) const { return d * (L + 1) + i; }
};

// pred(n) for the set bits bit0 + n of a pair mask with n in [lo, hi], ascending, until one holds (-> true).  The kept pairs are
// ~7 % of the cells: a walk over the set bits of a run visits a few of them where a loop over its positions tests up to W.
template <class F>
ELEMDP_HOSTDEV bool any_mask_bit(const uint32_t* m, int bit0, int lo, int hi, F&& pred) {
  if (hi < lo) return false;
  const int b = bit0 + lo, e = bit0 + hi;
  int w = b >> 5;
  uint32_t word = m[w] & (~0u << (b & 31));
  for (;;) {
    while (word) {
      const int bit = (w << 5) + __builtin_ctz(word);
      if (bit > e) return false;
      if (pred(bit - bit0)) return true;
      word &= word - 1;
    }
    if (((w + 1) << 5) > e) return false;
    word = m[++w];
  }
}

// inside-liveness bits of cell (i, d) from the rows below it (UB_L: the loop chain exists everywhere)
ELEMDP_HOSTDEV int useful_inside_cell(const UsefulCtx& q, const uint8_t* m, int i, int d) {
  const int j = i + d;
  const bool pok = q.pair_ok(i, d), lok = q.left_ok(i, d), mok = q.m_ok(i, d), eok = q.e_ok(i, d);
  const int dmi = q.dmin[i];
  int r = UB_L | (pok ? UB_P : 0) | (eok ? UB_E : 0);
  bool iA = false;
  if (dmi > 0 && dmi < d) {           // (the pair entries of the factorised rule 2 exist)
    if (dmi < d - 1 && q.unp[j - 1] && (m[q.at(i, d - 1)] & UB_A)) iA = true;             // tail step
    if (!iA)                                                                              // stems (j - sp, j), sp <= d - dmin[i]
      iA = any_mask_bit(q.okbits_end, j * (q.W + 1), 1, d - dmi, [&](int sp) { return (m[q.at(i, d - sp)] & UB_1) != 0; });
  }
  const bool iB = lok && iA;
  const bool do2 = lok && d > 0 && q.left_ok(i, d - 1) && q.unp[j - 1];
  const bool i2 = lok && (pok || (do2 && (m[q.at(i, d - 1)] & UB_2)));
  const bool doM = mok && q.m_ok(i + 1, d - 1) && q.unp[i];
  const bool iM = mok && (iB || (doM && (m[q.at(i + 1, d - 1)] & UB_M)));
  return r | (iA ? UB_A : 0) | (iB ? UB_B : 0) | (i2 ? UB_2 : 0) | ((i2 || iB) ? UB_1 : 0) | (iM ? UB_M : 0);
}

// The loops L(i, k) and L(l, j) that an interior loop of the E cell (i, d) reads, over the OUTSIDE enumeration (enum_interior:
// k - i <= C, whatever j - l) bounded by the loop size alone -- the superset of the plan's items that needs neither the energy
// tables nor the bases: calls f(cell index) for both operands of every candidate.
template <class F>
ELEMDP_HOSTDEV void useful_loop_operands(const UsefulCtx& q, int i, int d, F&& f) {
  if (!q.e_ok(i, d)) return;
  const int j = i + d;
  for (int l = j; l >= i + 2; --l) {
    int kmax = (l - 2 < i + q.C) ? l - 2 : i + q.C;
    const int kcap = i + q.loop_cap - (j - l);
    if (kcap < kmax) kmax = kcap;
    if (kmax < i) break;
    const int shi = (l - i < q.W) ? l - i : q.W;       // spans l - k of the candidates k = i .. kmax: one run of bits at end l
    any_mask_bit(q.okbits_end, l * (q.W + 1), l - kmax, shi, [&](int sp) {
      const int k = l - sp;
      if (k == i && l == j) return false;
      f(q.at(i, k - i));
      f(q.at(l, j - l));
      return false;
    });
  }
}

// final bits of cell (i, d): m holds the final bits of the rows above and the inside bits of this row; lm[cell] != 0 where
// useful_loop_operands marked the cell
ELEMDP_HOSTDEV int useful_outside_cell(const UsefulCtx& q, const uint8_t* m, const uint8_t* lm, int i, int d) {
  const int j = i + d, W = q.W, L = q.L;
  const int in = m[q.at(i, d)];
  const bool lok = q.left_ok(i, d), mok = q.m_ok(i, d), eok = q.e_ok(i, d);
  const int dmi = q.dmin[i];
  const bool doM = mok && q.m_ok(i - 1, d + 1) && q.unp[i > 0 ? i - 1 : 0];
  const bool uM = (in & UB_M) && (eok || (doM && (m[q.at(i - 1, d + 1)] & UB_M)));         // rules 6a, 5a
  bool u1 = false;
  if ((in & UB_1) && lok) {                                                                 // rule 2: stems (j, j + sp)
    const int hi = (W - d < L - j) ? W - d : L - j;
    u1 = any_mask_bit(q.okbits, j * (W + 1), 1, hi, [&](int sp) { return (m[q.at(i, d + sp)] & UB_A) != 0; });
  }
  const bool uB = (in & UB_B) && (uM || u1);                                                // rules 5b, 4b
  const bool step = d + 1 <= W && j < L && q.unp[j];
  const bool uA = (in & UB_A) && dmi > 0 && dmi < d && (uB || (step && (m[q.at(i, d + 1)] & UB_A)));
  const bool do2 = lok && q.left_ok(i, d + 1) && q.unp[j];
  const bool u2 = (in & UB_2) && (u1 || (do2 && (m[q.at(i, d + 1)] & UB_2)));               // rules 4a, 3a
  const bool doL = j < L && d + 1 <= W;
  const bool uL = eok || lm[q.at(i, d)] != 0 || (doL && (m[q.at(i, d + 1)] & UB_L));        // rules 6b, 6c, L <- L
  return (in & (UB_P | UB_E)) | (uM ? UB_M : 0) | (uB ? UB_B : 0) | (uA ? UB_A : 0) | (u1 ? UB_1 : 0) | (u2 ? UB_2 : 0) | (uL ? UB_L : 0);
}

// the whole mask of one sequence, serially (the host entry elemdp_useful_mask_host; the GPU runs the same cell functions with
// the cells of a diagonal dealt to the lanes of a workgroup: k_useful_mask, kernels.hip).  m, lm: (W+1) * (L+1) bytes each.
ELEMDP_HOSTDEV void useful_mask_serial(const UsefulCtx& q, uint8_t* m, uint8_t* lm) {
  const int L = q.L, W = q.W, n = (W + 1) * (L + 1);
  for (int c = 0; c < n; ++c) { m[c] = 0; lm[c] = 0; }
  for (int d = 0; d <= W && d <= L; ++d)
    for (int i = 0; i + d <= L; ++i) m[q.at(i, d)] = (uint8_t)useful_inside_cell(q, m, i, d);
  for (int d = 0; d <= W && d <= L; ++d)
    for (int i = 0; i + d <= L; ++i) useful_loop_operands(q, i, d, [&](int c) { lm[c] = 1; });
  for (int d = (W < L ? W : L); d >= 0; --d)
    for (int i = 0; i + d <= L; ++i) m[q.at(i, d)] = (uint8_t)useful_outside_cell(q, m, lm, i, d);
}

// ---------------------------------------------------------------------------------------------
// Pair terms: which terms 1(i,k) x stem (k,j) -> A(i,j) of the factorised rule 2 can be non-zero, as the outside
// sweep walks them -- two 64-bit words per cell from the finished mask `m` ([d][i]), the pair mask and dmin; W <= 64
// (kPairTermsMaxW, kernels.h).  Both words hold the same set of triples (i, k, j): ha_rows by the stem cell (k, j - k), h1_stems
// by the left cell (i, k - i).
// ---------------------------------------------------------------------------------------------

// the parent rows of the stem cell (i, d): bit b - 1, 1 <= b <= W - d, is set where 1(i - b, i) is parsable (the kernel's `ok`),
// A(i - b, i + d) has UB_A and 1(i - b, i) has UB_1; 0 where (i, d) is no kept pair
ELEMDP_HOSTDEV unsigned long long ha_rows(const UsefulCtx& q, const uint8_t* m, int i, int d) {
  if (!q.pair_ok(i, d)) return 0ull;
  unsigned long long w = 0ull;
  for (int b = 1; b <= q.W - d && b <= i; ++b) {
    const int ii = i - b, dm = q.dmin[ii];
    if (dm > 0 && b >= dm && (m[q.at(ii, d + b)] & UB_A) && (m[q.at(ii, b)] & UB_1)) w |= 1ull << (b - 1);
  }
  return w;
}

// the stems that start at the end j = i + d of the cell (i, d): bit sp - 1, 1 <= sp <= min(W - d, L - j), is set where (j, sp) is
// a kept pair and A(i, j + sp) has UB_A; 0 where 1(i, j) is not parsable or has no UB_1
ELEMDP_HOSTDEV unsigned long long h1_stems(const UsefulCtx& q, const uint8_t* m, int i, int d) {
  if (!q.left_ok(i, d) || !(m[q.at(i, d)] & UB_1)) return 0ull;
  const int j = i + d, hi = (q.W - d < q.L - j) ? q.W - d : q.L - j;
  unsigned long long w = 0ull;
  any_mask_bit(q.okbits, j * (q.W + 1), 1, hi, [&](int sp) {
    if (m[q.at(i, d + sp)] & UB_A) w |= 1ull << (sp - 1);
    return false;
  });
  return w;
}

}  // namespace elemdp
