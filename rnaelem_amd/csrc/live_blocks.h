// live_blocks.h -- the live-block lists of the train sweeps: the rule that forms them and where they lie in the plan.  Plain C++,
// host and device: the list kernel (kernels.hip), the band kernels (lin_kernels.hip), the host entry of the C ABI and the engine.
#pragma once
#include <cstdint>

// (functions that run on the host too, where the recurrences of dp_rules.h are device code only)
#if defined(__HIPCC__)
#define ELEMDP_HOSTDEV __host__ __device__ __forceinline__
#else
#define ELEMDP_HOSTDEV inline
#endif

namespace elemdp {

// ---------------------------------------------------------------------------------------------
// Live blocks: the cells of a diagonal d <= W that a workgroup of the table-driven train kernels sweeps, as a list
// of the cells with a non-zero mask byte instead of `cpb` consecutive ones.  The non-zero bytes of the diagonal are walked in
// ascending i; a block takes the next live cell until it has `cpb` of them, the next live cell lies `cap` or more cells behind
// its first (the context window a workgroup stages covers `cap` cells), or the diagonal ends.  cap >= cpb, so every block but
// the last of a diagonal spans at least cpb cells: at most ceil(ncell / cpb) blocks, the grid that exists.
// A block OWNS the cells from its first live cell up to the next block's first (the first block also the dead cells in front,
// the last one those behind): the owned ranges partition 0 .. ncell - 1, and a block stores the zeros of the dead cells it owns.
// A diagonal without a live cell has no block.
// `bits`: the planes that make a cell live (UB_* of plan_rules.h; default: any).  The inside sweep whose L plane a row pre-pass has
// filled (option loop_prepass) takes the lists of `~UB_L`: a cell that is useful in the L plane alone has nothing left to compute.
// ---------------------------------------------------------------------------------------------
constexpr int kLiveSpanMax = 64;   // largest `cap`: the live cells of a block are the set bits of one 64-bit word
constexpr int kLiveSpanDefault = 32;   // the default (option live_span): the largest at which the train kernels keep their workgroups per CU at W = 50
struct LiveBlock {
  uint64_t live;                   // bit k: cell first + k is live (bit 0 always; the highest set bit < cap; `count` bits)
  int16_t first;                   // the block's first live cell
  int16_t own_lo, own_end;         // the block owns the cells [own_lo, own_end)
  int16_t count;                   // live cells, 1 .. cpb
};
// the blocks of one diagonal from its mask bytes row[0 .. ncell); out: room for ceil(ncell / cpb) records; returns their number
ELEMDP_HOSTDEV int live_blocks_row(const uint8_t* row, int ncell, int cpb, int cap, LiveBlock* out, int bits = 0xff) {
  int nb = 0;
  LiveBlock b{0, 0, 0, 0, 0};
  for (int i = 0; i < ncell; ++i) {
    if (!(row[i] & bits)) continue;
    if (b.count == 0 || b.count == cpb || i - b.first >= cap) {
      if (b.count) { b.own_end = (int16_t)i; out[nb++] = b; }
      b.live = 1ull; b.first = (int16_t)i; b.own_lo = (int16_t)(nb == 0 ? 0 : i); b.count = 1;
    } else {
      b.live |= 1ull << (i - b.first);
      ++b.count;
    }
  }
  if (b.count) { b.own_end = (int16_t)ncell; out[nb++] = b; }
  return nb;
}
// the workgroups of cpb CONSECUTIVE cells of the diagonal that hold a live cell (the ones that do work without lists)
ELEMDP_HOSTDEV int working_blocks_row(const uint8_t* row, int ncell, int cpb, int bits = 0xff) {
  int n = 0;
  for (int i0 = 0; i0 < ncell; i0 += cpb) {
    bool any = false;
    for (int i = i0; i < ncell && i < i0 + cpb; ++i) any = any || (row[i] & bits) != 0;
    n += any;
  }
  return n;
}
// A diagonal takes its lists where they leave at most this share of the workgroups that work without them: a listed block pays
// for its record and, where its cells are not consecutive, for their offsets (measured: 2 - 4 % of a launch whose blocks the
// lists do not make fewer)
constexpr int kLiveKeepPct = 92;
// Where the lists of a sequence lie (records of 16 bytes from SeqPlan::blk_base on): W + 1 headers -- the block count of each
// diagonal in `count`, the rest 0 --, then live_blocks_slots(L) records per diagonal.  The room is set aside with the plan, before
// the geometry of the sweeps is known: enough for every cpb >= kLiveCpbMin (a launch with fewer cells per block takes no lists).
constexpr int kLiveCpbMin = 8;
ELEMDP_HOSTDEV int live_blocks_slots(int L) { return (L + kLiveCpbMin) / kLiveCpbMin; }                 // ceil((L + 1) / kLiveCpbMin)
ELEMDP_HOSTDEV long long live_blocks_records(int L, int W) { return (long long)(W + 1) * (1 + live_blocks_slots(L)); }
ELEMDP_HOSTDEV long long live_blocks_at(int L, int W, int d) { return (W + 1) + (long long)d * live_blocks_slots(L); }
// The plan holds TWO such sets per sequence, each of all its records: the lists of the whole byte (the outside sweep, and the
// inside sweep without the pre-pass) at PlanArrays::blocks, the lists of the inside sweep behind the pre-pass (the byte without its
// L bit) at PlanArrays::blocks_in = blocks + the records of the whole plan.
constexpr int kLiveInsideBits = 0x7f;   // UB_ALL & ~UB_L (plan_rules.h asserts it)
// The first diagonal on which an entry outside the L plane can be parsable at all: E(i, d) closes a pair of span d + 2 >= min_span
// (e_ok), P, B, 1 and 2 need a pair of span d >= min_span (pair_ok, left_ok through dmin), M needs d >= m_min (m_ok).  Below it
// the inside sweep behind the pre-pass has nothing to compute and nothing to store.
ELEMDP_HOSTDEV int first_inside_diagonal(int min_span, int m_min) {
  const int e = min_span - 2, d = e < m_min ? e : m_min;
  return d > 0 ? d : 0;
}

}  // namespace elemdp
