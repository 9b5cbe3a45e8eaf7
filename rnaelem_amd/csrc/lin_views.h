// lin_views.h -- the views of one table slot of the scaled-linear sweeps (model, sequence, inside / outside tables), device code
// shared by the band kernels (lin_kernels.hip) and the sampler (sample_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>

#include "dp_rules.h"
#include "kernels.h"

namespace elemdp {

struct LViews {
  ModelView m;
  // `lay` must live in LDS (stage_layout): every field access of a layout in global memory is a vector load with its
  // own wait, dozens of serialized round trips per target
  __device__ explicit LViews(const AutomatonLayout& lay) : m(lay) {}
  SeqView q;
  TableView in, out;
  int n;
  bool positive;
  long long seq_base, pos_base;
  double* row;
  double* zs;
};

__device__ __forceinline__ void make_lviews(const LinArgs& a, int g, LViews& v) {
  // the plan of the slot: one uniform record (g is the same for the whole workgroup: scalar loads), no grp -> plans chain
  // (read through the constant address space: the record is not written while kernels run, and a uniform address then
  // becomes scalar loads -- one wait for the whole record)
  g = __builtin_amdgcn_readfirstlane(g);
#if defined(__HIP_DEVICE_COMPILE__)
  typedef const SeqPlan __attribute__((address_space(4))) * ConstPlan;
  const SeqPlan p = *reinterpret_cast<ConstPlan>(reinterpret_cast<uintptr_t>(a.plans_slot + g));
#else
  const SeqPlan p = a.plans_slot[g];
#endif
  const int n = p.index;
  v.n = n;
  v.positive = p.positive != 0;
  v.seq_base = p.seq_base;
  v.pos_base = p.pos_base;
#if defined(__HIP_DEVICE_COMPILE__)
  typedef const ParamBlock __attribute__((address_space(4))) * ConstParams;   // (uniform, read-only: scalar loads)
  const ParamBlock pbv = *reinterpret_cast<ConstParams>(reinterpret_cast<uintptr_t>(a.params));
#else
  const ParamBlock pbv = *reinterpret_cast<const ParamBlock*>(a.params);
#endif
  const ParamBlock* pb = &pbv;
  v.m.ints = a.ints;
  v.m.big = a.ints;
  v.m.theta = a.params + sizeof(ParamBlock) / sizeof(double);
  v.m.lin = a.lin;
  v.m.lambda[0] = pb->lambda[0];
  v.m.lambda[1] = pb->lambda[1];
  v.m.log_tau = pb->log_tau;
  v.m.lam_same = pb->lam_same;
  v.m.no_prf = a.no_prf;
  v.m.m_min = a.m_min;
  v.m.dbg = a.dbg;
  SeqView& q = v.q;
  q.L = p.L; q.W = p.W; q.C = p.C;
  q.seq = a.b.seq + p.seq_base;
  q.ws = a.b.ws + p.pos_base;
  q.ews = a.ews + p.pos_base;
  q.unp = a.b.unp + p.pos_base;
  q.okbits = a.okbits + p.bits_base;
  q.dmin = a.p.dmin + p.dmin_base;
  q.e_stack = a.p.e_stack + p.cell_base; q.e_ext = a.p.e_ext + p.cell_base; q.e_ml = a.p.e_ml + p.cell_base;
  q.e_close = a.p.e_close + p.cell_base; q.e_hp = a.p.e_hp + p.cell_base;
  q.xwc = a.xwc + p.cell_base; q.xwc_stride = a.xwc_stride;
  q.xwi = a.xwi + p.item_base; q.xwi_stride = a.xwi_stride;
  q.items_inner = a.p.items_inner + p.item_base; q.items_left = a.p.items_left + p.item_base;
  q.items_right = a.p.items_right + p.item_base;
  q.items = a.p.items + p.item_base; q.item_in = a.p.item_in + p.item_base;
  q.by_outer_off = a.p.by_outer_off + p.off_base;
  q.by_inner_off = a.p.by_inner_off + p.off_base; q.by_inner_idx = a.p.by_inner_idx + p.item_base;
  q.by_left_off = a.p.by_left_off + p.off_base; q.by_left_idx = a.p.by_left_idx + p.item_base;
  q.by_right_off = a.p.by_right_off + p.off_base; q.by_right_idx = a.p.by_right_idx + p.item_base;
  v.in.band = a.band_in + (size_t)g * a.band_stride;
  v.in.ext = a.ext_in + (size_t)g * a.ext_stride;
  v.out.band = a.band_out + (size_t)g * a.band_stride;
  v.out.ext = a.ext_out + (size_t)g * a.ext_stride;
  v.in.L = v.out.L = p.L; v.in.W = v.out.W = p.W; v.in.S = v.out.S = a.lay.S;
  v.in.ap = a.a_in ? a.a_in + (size_t)g * a.a_stride : nullptr;
  v.out.ap = a.a_out ? a.a_out + (size_t)g * a.a_stride : nullptr;
  v.in.nA = v.out.nA = a.lay.n_ap;
  v.in.set_compact(a.lay, a.ints);      // (the column map moves to LDS with the automaton blob: stage_context)
  v.out.set_compact(a.lay, a.ints);
  v.in.cyk_compact = a.cyk_compact;      // (the Viterbi pass sweeps band_in: TableView::ldm / stm)
  q.okbits_end = a.okbits_end ? a.okbits_end + p.bits_base : nullptr;
  q.useful = a.p.useful ? a.p.useful + p.cell_base : nullptr;
  q.blocks = a.p.blocks ? a.p.blocks + p.blk_base : nullptr;
  q.ha_rows = a.p.ha_rows ? a.p.ha_rows + p.cell_base : nullptr;
  q.h1_stems = a.p.ha_rows ? a.p.h1_stems + p.cell_base : nullptr;
  v.row = a.seq_out + (size_t)n * a.out_stride;
  v.zs = a.zs + (size_t)g * 4;
}

}  // namespace elemdp
