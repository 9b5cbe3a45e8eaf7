// stem_rules.h -- pair posteriors by motif node pair and the pair counts behind a stem logo, host / device.
//
// A pair transition s -> sp of the flattened automaton emits the two bases of a pair jointly: the left base i by node st_l(sp),
// the right base j-1 by node st_r(s) (node_rules.h routes the same transition to one node or to the other).  A stem slot is a
// distinct node pair (ml, mr) = (st_l(sp), st_r(s)) over these transitions, slots in increasing (ml, mr) order, K of them.  For a
// kept cell [i, j), d = j - i >= 2, over the ensemble of the scan's first sum pass (terminals ari and nasi, Z = Z(ari, nasi): the
// ensemble of pair_rules.h and node_rules.h):
//
//   Q(i, d, k) = sum over the transitions (s, sp, tf) of slot k:
//                   out(P, i, d, s) wp(s, sp, tf, i, j-1) ( in(E, i+1, d-2, sp)  +  in(P, i+1, d-2, sp) xst(s, cell) ) / Z
//                                                           rule 1a                  rule 1b, under pair_ok(i+1, d-2)
//
// with the guards of node_pairs: the caller holds pair_ok(i, d) and d >= 2; an out(P) entry that is dead ends its term before
// any further load.  Every entry is clamped to [0, 1]; nothing is renormalised.  sum_k Q(i, d, k) is the P of pair_rules.h
// wherever the tables' inside and outside agree, and the sums of Q over the slots with one left (right) node are the pair-left
// (pair-right) parts of node_rules.h.  A cell that is not kept, and every cell with d < 2, has Q = 0.
//
// Counts: C[k][bl][br] = sum over the kept cells of Q(i, d, k) [seq[i] = bl] [seq[j-1] = br], base codes N A C G U, rows i in
// increasing order and within a row d in increasing order.  A sequence without any parse, and every sequence of a model
// without secondary structure (ELEMDP_NO_RSS), has no Q at all: its counts are 0, its list is empty, the band tables are not read.
//
// Q of one table slot is kept by stem slot, then by d, then by i (stem_at): the lanes of k_stem_cells, i fastest, write
// neighbouring doubles.  One rule for both forms (StemLin / StemLog); w_pair2 and w_stack are those of NodeLin / NodeLog.
#pragma once
#include <utility>
#include <vector>

#include "node_rules.h"
#include "pair_rules.h"

namespace elemdp {

constexpr int kStemBases = 5;                            // N A C G U
constexpr int kStemBlock = kStemBases * kStemBases;      // one slot's counts: [bl][br]
constexpr int kStemMaxSlots = 255;
// the two terms of Q as bits of StemLists::parts (both in the product; the CPU driver of the tests drops one to show that its
// references see each)
enum StemPart : int { SP_1A = 1, SP_1B = 2, SP_ALL = 3 };

struct StemLists {
  const int32_t* v;   // K + 1 offsets (entry indices), 2 K node indices (ml, mr per slot), then the entries, 3 ints each (s, sp, tf)
  int32_t K;
  int32_t parts;      // StemPart bits
  ELEMDP_HD int begin(int k) const { return v[k]; }
  ELEMDP_HD int end(int k) const { return v[k + 1]; }
  ELEMDP_HD int left(int k) const { return v[K + 1 + 2 * k]; }
  ELEMDP_HD int right(int k) const { return v[K + 2 + 2 * k]; }
  ELEMDP_HD const int32_t* ent(int e) const { return v + 3 * K + 1 + 3 * e; }
};

// the blob StemLists reads, from a flattened automaton (host); returns K.  Within a slot the transitions keep the automaton's
// order (parent state, then its pair list).
inline int stem_lists_build(const AutomatonLayout& A, const int32_t* I, std::vector<int32_t>* blob) {
  struct Ent { int ml, mr, s, sp, tf; };
  std::vector<Ent> ents;
  std::vector<std::pair<int, int>> slots;
  for (int s = 0; s < A.S; ++s)
    for (int t = I[A.pair_off + s]; t < I[A.pair_off + s + 1]; ++t) {
      const int sp = I[A.pair_ent + 2 * t];
      ents.push_back({I[A.st_l + sp], I[A.st_r + s], s, sp, I[A.pair_ent + 2 * t + 1]});
    }
  for (int ml = 0; ml < A.M; ++ml)
    for (int mr = 0; mr < A.M; ++mr)
      for (const Ent& e : ents)
        if (e.ml == ml && e.mr == mr) { slots.push_back({ml, mr}); break; }
  const int K = (int)slots.size();
  blob->assign((size_t)3 * K + 1, 0);
  int n = 0;
  for (int k = 0; k < K; ++k) {
    (*blob)[k] = n;
    (*blob)[K + 1 + 2 * k] = slots[k].first;
    (*blob)[K + 2 + 2 * k] = slots[k].second;
    for (const Ent& e : ents)
      if (e.ml == slots[k].first && e.mr == slots[k].second) { blob->push_back(e.s); blob->push_back(e.sp); blob->push_back(e.tf); ++n; }
  }
  (*blob)[K] = n;
  return K;
}

struct StemLin : NodeLin {
  ELEMDP_HD explicit StemLin(double invZ_) : NodeLin(invZ_) {}
};
struct StemLog : NodeLog {
  ELEMDP_HD explicit StemLog(double lnZ_) : NodeLog(lnZ_) {}
};

// where Q(i, d, k) of a sequence lies in the per-slot scratch of its table slot
ELEMDP_HD size_t stem_at(int L, int W, int k, int i, int d) { return ((size_t)k * (W + 1) + d) * (size_t)(L + 1) + i; }
// doubles of that scratch (host)
inline size_t stem_scratch_size(int Lmax, int Wmax, int K) { return ((size_t)Lmax + 1) * ((size_t)Wmax + 1) * (size_t)(K > 0 ? K : 1); }

// Q(i, d, k) of the kept cell [i, i + d), d >= 2, i + d <= L (the caller checked pair_ok(i, d))
template <class F>
ELEMDP_HD double stem_cell(const F& f, const StemLists& sl, const ModelView& m, const SeqView& q, const TableView& in,
                           const TableView& out, int d, int i, int k) {
  const bool cP = q.pair_ok(i + 1, d - 2);
  double a = 0.;
  for (int e = sl.begin(k); e < sl.end(k); ++e) {
    const int32_t* t = sl.ent(e);
    const int s = t[0], sp = t[1];
    const double o = f.ld(out, ST_P, d, i, s);
    if (f.dead(o)) continue;
    const double ow = f.mul(o, f.w_pair2(m, q, s, sp, t[2], i, i + d - 1));
    if (sl.parts & SP_1A) a += f.post(f.mul(ow, f.ld(in, ST_E, d - 2, i + 1, sp)));                                                  // 1a
    if (cP && (sl.parts & SP_1B)) a += f.post(f.mul(ow, f.mul(f.ld(in, ST_P, d - 2, i + 1, sp), f.w_stack(m, q, s, q.cell(i, d)))));   // 1b
  }
  return ctx_clamp(a);
}

// Q(i, d, k) of any cell with i + d <= L: 0 where the cell is not kept or too short to pair
template <class F>
ELEMDP_HD double stem_value(const F& f, const StemLists& sl, const ModelView& m, const SeqView& q, const TableView& in,
                            const TableView& out, int d, int i, int k) {
  return d >= 2 && q.pair_ok(i, d) ? stem_cell(f, sl, m, q, in, out, d, i, k) : 0.;
}

// a value every lane of a wave holds alike, kept in a scalar register on the device (stem_count walks the pair mask with it)
ELEMDP_HD uint32_t stem_uniform(uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
  return (uint32_t)__builtin_amdgcn_readfirstlane((int)v);
#else
  return v;
#endif
}

// counts[(k 5 + bl) 5 + br] of one sequence for entry t: the kept cells in the order of their mask bits (rows in increasing i,
// within a row increasing d), found by walking the set bits of the mask words.  The lanes of a wave must call it for the same
// sequence: the walk is then scalar work, and a lane only adds where the two bases of the cell are its own.  Each value is
// added one match later than it is loaded, so the load of a match is in flight while the mask is walked on.
ELEMDP_HD double stem_count(const double* X, const uint8_t* seq, const uint32_t* okbits, int L, int W, int t) {
  const int bin = t % kStemBlock, k = t / kStemBlock;
  const int ncell = (L + 1) * (W + 1);
  double a = 0., cur = 0.;
  for (int c0 = 0; c0 < ncell; c0 += 32) {
    uint32_t w = stem_uniform(okbits[c0 >> 5]);
    while (w) {
      const int c = c0 + __builtin_ctz(w);
      w &= w - 1;
      const int i = c / (W + 1), d = c - i * (W + 1);
      if (d < 2 || i + d > L) continue;
      if (seq[i] * kStemBases + seq[i + d - 1] != bin) continue;
      a += cur;
      cur = X[stem_at(L, W, k, i, d)];
    }
  }
  return a + cur;
}

}  // namespace elemdp
