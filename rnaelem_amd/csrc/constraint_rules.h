// constraint_rules.h -- hard structure constraints per sequence, host/device agnostic.
//
// A constraint string has one character per base, ViennaRNA's alphabet:
//   .  free            x  must be unpaired        |  must be paired (any partner)
//   <  paired, the 5' base of its pair            >  paired, the 3' base of its pair
//   ( )  these two bases pair with each other (balanced, nested)
// The host derives per position (constraint_derive, host_prep.h) a class byte, partner[p] (the other base of a forced pair, else
// -1) and enc[p], the opening base of the innermost forced pair that STRICTLY encloses p (-1: none; for the two bases of a
// forced pair that is the pair around their own).  From these the rule below says which pair cells survive; the rest of the
// constrained ensemble follows from the `unp` row (class '.' or 'x': the position may be emitted unpaired) and the `ndot` row
// (prefix counts of the positions that must pair) the DP rules and the plan builder already honour.
// The functions are host and device code under hipcc too (ELEMDP_HOSTDEV, not the device-only ELEMDP_HD of the recurrences): the
// engine checks the strings and serves elemdp_constraint_mask_host with them on the CPU.
#pragma once
#include "dp_rules.h"
#include "live_blocks.h"

namespace elemdp {

enum ConsClass : uint8_t { CONS_FREE = 0, CONS_X = 1, CONS_PAIRED = 2, CONS_LEFT = 3, CONS_RIGHT = 4, CONS_OPEN = 5, CONS_CLOSE = 6 };

// class of a constraint character, -1: not in the alphabet
ELEMDP_HOSTDEV int cons_class(char c) {
  switch (c) {
    case '.': return CONS_FREE;
    case 'x': return CONS_X;
    case '|': return CONS_PAIRED;
    case '<': return CONS_LEFT;
    case '>': return CONS_RIGHT;
    case '(': return CONS_OPEN;
    case ')': return CONS_CLOSE;
  }
  return -1;
}

// the rows of one sequence (L entries each)
struct ConsView {
  const uint8_t* cls;
  const int32_t* partner;
  const int32_t* enc;
};

// may position p be emitted unpaired?
ELEMDP_HOSTDEV bool cons_unp(int cls) { return cls == CONS_FREE || cls == CONS_X; }

// the pair of bases i < r is one of the forced pairs
ELEMDP_HOSTDEV bool cons_forced(const ConsView& c, int i, int r) { return c.cls[i] == CONS_OPEN && c.partner[i] == r; }

// May bases i < r pair under the constraint?
//   * neither is 'x';
//   * i may be a 5' base: '.', '|', '<', or the '(' whose ')' is r;      r may be a 3' base: '.', '|', '>', or the ')' of i;
//   * the pair crosses no forced pair (a, b): neither a < i < b < r nor i < a < r < b.
// For the last test enc[i] == enc[r] suffices once the first two have passed.  They leave two cases.  Either (i, r) is a forced
// pair itself: it crosses none (the string is nested), and enc of both bases is the pair around it.  Or neither base belongs to a
// forced pair: then (a, b) is crossed iff exactly one of i, r lies strictly inside it, that is iff the sets of forced pairs that
// strictly enclose i and r differ; nested pairs form a forest, the set of a position is the chain from its innermost pair to the
// root, and two chains are equal iff they start at the same pair.  (A '(' or ')' at one end only never passes the class tests:
// its partner is another base.)
ELEMDP_HOSTDEV bool cons_allowed(const ConsView& c, int i, int r) {
  const int ci = c.cls[i], cr = c.cls[r];
  if (ci == CONS_X || cr == CONS_X) return false;
  if (!(ci == CONS_FREE || ci == CONS_PAIRED || ci == CONS_LEFT || c.partner[i] == r)) return false;
  if (!(cr == CONS_FREE || cr == CONS_PAIRED || cr == CONS_RIGHT || c.partner[r] == i)) return false;
  return c.enc[i] == c.enc[r];
}

// One 32-bit word of the pair mask of a sequence (bit c = i * (W+1) + d <=> pair cell (i, d), bases i and i + d - 1) under the
// constraint: the filter's bits that are allowed, and the forced pairs of the word's rows.  Bits that stand for no cell stay.
ELEMDP_HOSTDEV uint32_t cons_word(const ConsView& c, int L, int W, int w, uint32_t in) {
  const int W1 = W + 1;
  uint32_t out = in;
  for (uint32_t m = in; m; m &= m - 1) {
    const int k = __builtin_ctz(m);
    const int cell = w * 32 + k;
    const int i = cell / W1, d = cell - i * W1;
    if (d >= 1 && i + d <= L && !cons_allowed(c, i, i + d - 1)) out &= ~(1u << k);
  }
  const int c0 = w * 32, c1 = c0 + 31;
  int ihi = c1 / W1;
  if (ihi > L - 1) ihi = L - 1;
  for (int i = c0 / W1; i <= ihi; ++i) {
    if (c.cls[i] != CONS_OPEN) continue;
    const int cell = i * W1 + (c.partner[i] - i + 1);   // (the span is at most W: constraint_derive refuses wider pairs)
    if (cell >= c0 && cell <= c1) out |= 1u << (cell - c0);
  }
  return out;
}

}  // namespace elemdp
