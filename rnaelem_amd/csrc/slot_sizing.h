// slot_sizing.h -- how many table slots a call gets and how many sequences it sweeps in lockstep: plain functions of a request,
// the free device memory and the memory the handle already holds.  No HIP call and no Engine in here (TableSlots, engine.cpp,
// asks the device and passes the numbers in), so tests/slots_check.cpp drives the same code on the host.
#pragma once
#include <algorithm>
#include <cstddef>

#include "device_layout.h"

namespace elemdp {

// Everything that sizes the table slots of a call.
struct SlotRequest {
  int S = 0;           // interval states per row of the exterior tables
  int row = 0;         // doubles per cell of a band table (0: the dense layout, kNumBandStates * S)
  bool scan = false;   // the slots carry the trace rows and traceback stacks of the fused scan kernel
  int n_want = 0;      // sequences the call covers: it never gets more slots than that
  int group = 0;       // wanted slot count (a group size; 0: option `slots`, else twice the compute units)
  int opt_slots = 0, n_cu = 0;
  int pair_row = 0;    // a call of the scaled-linear pipeline: doubles per cell of its pair tables (factorised rule 2), at least 1;
                       // 0: a log-space call, which gets none of that pipeline's side buffers (scales, pair tables)
  int Lmax = 0, Wmax = 0;
  int S_dense = 0;     // states of the plain automaton: one DENSE table fits into the band buffers whatever the row
  size_t budget = 0;   // an inner handle of a streamed batch: the share of the device memory its slots stay in (0: none)

  size_t cells() const { return (size_t)(Wmax + 1) * (Lmax + 1); }
  size_t band() const { return cells() * (row > 0 ? row : kNumBandStates * S); }
  size_t ext() const { return (size_t)(Lmax + 1) * S; }
  size_t dense1() const { return (size_t)kNumBandStates * (Wmax + 1) * (Lmax + 1) * S_dense; }
  size_t per_slot() const {
    return (band() + ext()) * 2 * sizeof(double) + (scan ? ext() * sizeof(TraceRec) + 16 * (size_t)(Lmax + 2) : 0);
  }
  int want() const { return std::max(1, std::min(group > 0 ? group : opt_slots > 0 ? opt_slots : 2 * n_cu, n_want)); }
};

// What the slots were sized for.  trace: their budget counted the trace rows (a scan request sized them).
struct SlotGeometry {
  int n = 0, S = 0;
  bool trace = false;
  size_t band_stride = 0;
};

// int32 words of one slot's traceback stack
inline int trace_stack_stride(int Lmax) { return 4 * (4 * (Lmax + 2)); }

// The slots that are there serve the request: no fewer than it wants, the same row widths, trace tables if it asks for them.
// (More slots than wanted are kept: a load_batch per evaluation must not re-allocate the tables.)
inline bool slots_keep(const SlotGeometry& g, const SlotRequest& r) {
  return g.n >= r.want() && g.S == r.S && g.band_stride == r.band() && (g.trace || !r.scan);
}

// Slots of a fresh sizing: what the request wants, cut to 72 % of the memory within reach (free + held by the slot buffers) and
// to an inner handle's budget, at least one; 0 when not even one fits.
inline int slots_sized(const SlotRequest& r, size_t free_b, size_t held_b) {
  const size_t per_slot = r.per_slot();
  int want = r.want();
  size_t budget = (size_t)((double)(free_b + held_b) * 0.72);
  if (r.budget > 0) budget = std::min(budget, r.budget);
  if (per_slot * (size_t)want > budget) want = (int)std::max<size_t>(1, budget / per_slot);
  if (per_slot * want > free_b + held_b) return 0;
  return want;
}

// n sequences in groups of at most n_slots, all groups of the same size (a small last group runs at lower efficiency)
inline int even_groups(int n, long n_slots) {
  const long n_groups = (n + n_slots - 1) / n_slots;
  return (int)((n + n_groups - 1) / n_groups);
}

// Sequences swept in lockstep: option `group`, or as many as fit in 68 % of the memory within reach (at most group_cap, inside an
// inner handle's budget), then balanced over the groups of the batch.
inline int balanced_group(size_t per_slot_bytes, int n, int group_cap, int opt_group, size_t budget_in, size_t free_b, size_t held_b) {
  if (opt_group > 0) return opt_group;
  size_t budget = (size_t)((double)(free_b + held_b) * 0.68);
  if (budget_in > 0) budget = std::min(budget, budget_in);
  long cap = (long)(budget / std::max<size_t>(per_slot_bytes, 1));
  cap = std::max(1L, std::min(cap, (long)group_cap));
  return even_groups(n, cap);
}

// device memory per sequence of a group of the scaled-linear pipeline: band and exterior tables (Sa states), scratch rows, pair tables
inline size_t lin_group_bytes(int Lmax, int Wmax, int row, int Sa, int nap) {
  const size_t cells = (size_t)(Wmax + 1) * (Lmax + 1), ext = (size_t)(Lmax + 1);
  return (cells * row + ext * Sa) * 2 * sizeof(double) + ext * Sa * 3 * sizeof(double) + cells * nap * 2 * sizeof(double);
}

}  // namespace elemdp
