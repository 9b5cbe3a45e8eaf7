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

// The group size a sweep over ns streams ends up with: the n_slots slots are shared out evenly, every stream gets the same number
// of groups (one stream: gsz as it came).
inline int stream_group(int n, int gsz, int n_slots, int ns) {
  if (ns <= 1) return gsz;
  const int slots_each = std::max(1, n_slots / ns);
  int n_groups = (n + slots_each - 1) / slots_each;
  n_groups = ((n_groups + ns - 1) / ns) * ns;
  return (n + n_groups - 1) / n_groups;
}

// ---- a slot per sequence (option own_slots): an unranged train evaluation of a resident batch gives every sequence the slot of
// its position in processing order, so that what one evaluation leaves in a slot is still there for the next one of the same plan
// (the zeros of the dead entries: ZeroBinding).  The sequences swept in lockstep and the streams stay what they are without it.
//
// Do n sequences get a slot each?  Only inside both sizing rules -- the 68 % of balanced_group over a group's bytes per sequence
// and the 72 % of slots_sized over a slot's, each within an inner handle's budget -- and not where option `group` or `slots`
// asks for fewer slots than sequences.
inline bool own_slots_fit(int n, size_t group_bytes, size_t per_slot_bytes, int opt_group, int opt_slots, size_t budget_in, size_t free_b,
                          size_t held_group_b, size_t held_slots_b) {
  if (n < 1 || (opt_group > 0 && opt_group < n) || (opt_slots > 0 && opt_slots < n)) return false;
  auto inside = [&](size_t per, size_t reach, double frac) {
    size_t budget = (size_t)((double)reach * frac);
    if (budget_in > 0) budget = std::min(budget, budget_in);
    return per * (size_t)n <= budget;
  };
  return inside(group_bytes, free_b + held_group_b, 0.68) && inside(per_slot_bytes, free_b + held_slots_b, 0.72);
}
// the slots the groups of a sweep are cut for: with a slot per sequence still the `group` sequences of the shared mapping
inline int lockstep_slots(bool own, int group, int n, int n_slots) { return own ? std::max(1, std::min(group, n)) : n_slots; }
// first slot of the group that starts at position g0 of the processing order and runs on stream k (slots_each slots per stream)
inline size_t group_slot_base(bool own, int g0, int k, int slots_each) { return own ? (size_t)g0 : (size_t)k * slots_each; }

// "The dead entries of these slots hold the zeros of this binding": everything the set of entries the usefulness mask calls useless,
// and their addresses, depend on.  An evaluation whose binding matches the one the slots hold stores none of those zeros again
// (LinArgs::zeros_kept).
struct ZeroBinding {
  bool valid = false;              // false: the slots hold no such zeros (or the evaluation is none that could leave them)
  unsigned long long plan = 0;     // identity of the plan: bumped by load_batch and by whatever rebuilds the plan, its mask or its lists
  unsigned slots_gen = 0;          // the slots: their sizing generation, count, band stride; the mapping (a slot per sequence) and
  int n_slots = 0;                 // the sequences it covers
  size_t band_stride = 0;
  int own = 0, n_seq = 0;
  int S = 0, tab_row = 0, ap_rs = 0, shadow = 0, schedule = 0;   // the layout that was swept
  int useful_mask = 0, loop_prepass = 0, loop_outside = 0, live_blocks = 0, live_span = 0, deterministic = 0, fast = 0;   // options
};
// (option pair_terms is not compared: it drops terms of the outside pair sums that are exact zeros and were never added, so it
// changes no stored entry)
inline bool zeros_match(const ZeroBinding& held, const ZeroBinding& want) {
  return held.valid && want.valid && held.plan == want.plan && held.slots_gen == want.slots_gen && held.n_slots == want.n_slots &&
         held.band_stride == want.band_stride && held.own == want.own && held.n_seq == want.n_seq && held.S == want.S &&
         held.tab_row == want.tab_row && held.ap_rs == want.ap_rs && held.shadow == want.shadow && held.schedule == want.schedule &&
         held.useful_mask == want.useful_mask && held.loop_prepass == want.loop_prepass && held.loop_outside == want.loop_outside &&
         held.live_blocks == want.live_blocks && held.live_span == want.live_span && held.deterministic == want.deterministic &&
         held.fast == want.fast;
}

}  // namespace elemdp
