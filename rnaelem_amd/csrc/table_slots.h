// table_slots.h -- the table slots of an Engine (engine.cpp): their buffers, what they were sized for, what they hold.
#pragma once
#include "device_buf.h"
#include "slot_sizing.h"

namespace elemdp {

// The table slots of a handle: per slot the band and exterior tables of one sequence (inside and outside), scratch rows, and --
// for the calls that ask -- the pair tables of the factorised rule 2 or the trace tables of the fused scan kernel.  Every pipeline
// sweeps its groups over them.  ensure() is the one place that sizes them (slot_sizing.h has the arithmetic), from a request that
// carries every input; the geometry says what they were sized for, `holds` what the pipeline that ran last left in them.
struct TableSlots {
  // nothing a later call can read (fresh, invalidated, or behind the sum passes of a scan-family call); a train evaluation's log
  // values in dense tables, or its scaled linear values in compact tables; the fused scan kernel's tables with trace rows
  enum class Holds { Nothing, DenseLog, Linear, Trace };
  // which buffers a sizing rule counts as within its reach, next to the free memory (the three rules grew apart; each keeps its sum)
  enum class Held { Group, Slots, Stream };

  DevBuf band_in, band_out, ext_in, ext_out, tmp;
  DevBuf tr_ext, tr_stack;    // trace records of the exterior chain [Lmax+1][S_dense] and the traceback stack, per slot
  DevBuf zs, a_in, a_out;     // scaled-linear pipeline: scales, pair tables [W+1][Lmax+1][pair_row] per slot

  // slots a call may build on: none once they hold trace tables (the train pipelines do not reuse those)
  int n() const { return holds_ == Holds::Trace ? 0 : g_.n; }
  size_t band_stride() const { return g_.band_stride; }
  Holds holds() const { return holds_; }
  int linear_S() const { return linear_S_; }   // states per row of Holds::Linear tables (one more with the shadow state)
  // zeros: the binding whose dead entries the slots hold as zeros behind this call (a train evaluation's own record; anything
  // else that says what the slots hold leaves none)
  void set_holds(Holds h, int linear_S = 0, const ZeroBinding* zeros = nullptr) {
    holds_ = h; linear_S_ = linear_S;
    zeros_ = zeros ? *zeros : ZeroBinding();
  }
  // The zeros the slots hold (ZeroBinding::valid false: none).  A train evaluation TAKES the record before it touches the slots --
  // they then hold none until it sets its own --; ensure(), set_holds(), invalidate() and release() all drop it, so a call that
  // sweeps anything else over the slots cannot leave it standing.
  const ZeroBinding& zeros() const { return zeros_; }
  ZeroBinding take_zeros() { const ZeroBinding z = zeros_; zeros_ = ZeroBinding(); return z; }
  void clear_zeros() { zeros_ = ZeroBinding(); }
  unsigned generation() const { return gen_; }   // sizings so far: part of a ZeroBinding
  int n_held() const { return g_.n; }            // slots the buffers are sized for, whatever they hold

  size_t held_bytes(Held set) const {
    const size_t band = band_in.bytes() + band_out.bytes(), ext = ext_in.bytes() + ext_out.bytes();
    switch (set) {
      case Held::Group: return band + ext;
      case Held::Slots: return band + ext + tmp.bytes() + tr_ext.bytes() + tr_stack.bytes();
      default: return band;
    }
  }

  // Slots for the request, given the free device memory: what is there is kept if it serves (no reset -- DevBuf::alloc keeps what
  // is large enough), else sized afresh.  The pair tables follow the slot count in the same call.
  void ensure(const SlotRequest& r, size_t free_b) {
    clear_zeros();
    if (holds_ == Holds::Trace) invalidate();
    Lmax_ = r.Lmax; S_dense_ = r.S_dense;
    if (!slots_keep(g_, r)) {
      const int n = slots_sized(r, free_b, held_bytes(Held::Slots));
      if (n < 1) throw HipError("not enough device memory for one table slot");
      invalidate();   // (an allocation that fails below leaves no geometry behind)
      // (the log-space fallback of the scaled-linear pipeline sweeps dense tables over the same buffers: at least one fits)
      const size_t band = std::max(r.band() * n, r.dense1()) * sizeof(double);
      band_in.alloc(band);
      band_out.alloc(band);
      ext_in.alloc(r.ext() * n * sizeof(double));
      ext_out.alloc(r.ext() * n * sizeof(double));
      tmp.alloc(r.ext() * 3 * n * sizeof(double));
      g_.n = n; g_.S = r.S; g_.band_stride = r.band();
      if (r.scan) { ensure_trace(); g_.trace = true; }
    }
    if (r.pair_row > 0) {   // the side buffers of the scaled-linear pipeline (every call of it asks: SlotRequest::pair_row)
      zs.alloc(sizeof(double) * 4 * g_.n);
      a_in.alloc(sizeof(double) * r.cells() * r.pair_row * g_.n);
      a_out.alloc(sizeof(double) * r.cells() * r.pair_row * g_.n);
    }
  }
  // the scan's trace rows and traceback stacks for the slots that are there
  void ensure_trace() {
    tr_ext.alloc((size_t)(Lmax_ + 1) * S_dense_ * g_.n * sizeof(TraceRec));
    tr_stack.alloc((size_t)g_.n * trace_stack_stride(Lmax_) * sizeof(int32_t));
  }
  // keeps the memory, forgets what it was sized for and what it holds: the next ensure() sizes afresh
  void invalidate() { g_ = SlotGeometry(); ++gen_; set_holds(Holds::Nothing); }
  void release() {
    for (DevBuf* d : {&band_in, &band_out, &ext_in, &ext_out, &tmp, &tr_ext, &tr_stack, &zs, &a_in, &a_out}) d->reset();
    invalidate();
  }

 private:
  SlotGeometry g_;
  Holds holds_ = Holds::Nothing;
  ZeroBinding zeros_;
  unsigned gen_ = 0;
  int linear_S_ = 0, Lmax_ = 0, S_dense_ = 0;
};

}  // namespace elemdp
