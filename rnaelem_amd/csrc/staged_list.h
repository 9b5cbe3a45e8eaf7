// staged_list.h -- the batch lists of the posterior calls of an Engine (engine.cpp), their buffers and their format: StagedList, the
// one list of the pair, conditional, stem and helix calls, and LoopLists, the two lists of the loop call.  Host code only.
#pragma once
#include <cstdint>

#include "device_buf.h"
#include "kernels.h"
#include "loop_rules.h"

namespace elemdp {

// off[0 .. n] = exclusive prefix of cnt[0 .. n), queued on st; waits and returns the total off[n]
inline int64_t prefix_total(const DevBuf& cnt, int n, DevBuf& off, hipStream_t st) {
  HIP_OK(launch_pair_prefix(cnt.as<int64_t>(), n, off.as<int64_t>(), st));
  int64_t total = 0;
  HIP_OK(hipMemcpyAsync(&total, off.as<int64_t>() + n, sizeof(int64_t), hipMemcpyDeviceToHost, st));
  HIP_OK(hipStreamSynchronize(st));
  return total;
}
// a column of a list into the caller's (dst may be null: not asked for)
inline void fetch_column(void* dst, const DevBuf& src, size_t bytes) {
  if (dst) HIP_OK(hipMemcpy(dst, src.as<void>(), bytes, hipMemcpyDeviceToHost));
}

// One list of (sequence, i, j[, label]) entries with one or two value columns, built around the sweeps of a call:
//   begin()   kept cells per sequence -> prefix -> staging ranges of `mult` entries per kept cell (a sequence's list holds at most
//             that many); hands out the pointers the call's per-sequence kernel (k_pair_seq, k_cond_seq, k_stem_seq) writes a
//             sequence's entries and their number through;
//   finish()  prefix over the numbers -> one scatter out of the staging ranges into the batch list in (sequence, i, j[, label])
//             order, which stays on the device for fetch() until the next call of the same kind or the next load_batch.
// A streamed batch builds the list on the host instead, chunk by chunk (Host::append, adopt).  Every buffer is the list's own: a
// call leaves the lists of the other calls alone.  count() < 0: no list (invalidate()).
class StagedList {
 public:
  // list, call: the entry points' names in the refusals of fetch(); n_val: value columns, 1 or 2; label: a label column, one
  // byte per entry in staging, widened to int32 in the list
  StagedList(const char* list, const char* call, int n_val, bool label) : list_(list), call_(call), n_val_(n_val), label_(label) {}

  struct Staging {   // per batch index: first kept cell and entries written; then the columns of the staging ranges
    const int64_t* koff; int64_t* cnt;
    int32_t* st_i; int32_t* st_j; double* st_v[2]; uint8_t* st_k;
  };
  // Queues the kept-cell counts and their prefix for the n sequences of the resident batch on st, waits for the total, and
  // returns the staging ranges with every number of entries cleared.  (k_stem_seq would not need the clearing: it writes the
  // number of every sequence, in exactly one of the two forms of the call, 0 where it has no Q.  Clearing always is one rule.)
  Staging begin(const SeqPlan* plans, const uint32_t* okbits, int n, int mult, hipStream_t st) {
    n_ = n; mult_ = mult;
    kept_.alloc(8 * (size_t)n); koff_.alloc(8 * ((size_t)n + 1));
    cnt_.alloc(8 * (size_t)n); off_.alloc(8 * ((size_t)n + 1));
    HIP_OK(launch_pair_kept(plans, okbits, n, kept_.as<int64_t>(), st));
    const size_t cap = (size_t)prefix_total(kept_, n_, koff_, st) * (size_t)mult;
    st_i_.alloc(4 * cap); st_j_.alloc(4 * cap);
    for (int w = 0; w < n_val_; ++w) st_v_[w].alloc(8 * cap);
    if (label_) st_k_.alloc(cap);
    HIP_OK(hipMemsetAsync(cnt_.as<void>(), 0, 8 * (size_t)n, st));
    return Staging{koff_.as<int64_t>(), cnt_.as<int64_t>(), st_i_.as<int32_t>(), st_j_.as<int32_t>(),
                   {st_v_[0].as<double>(), n_val_ > 1 ? st_v_[1].as<double>() : nullptr}, label_ ? st_k_.as<uint8_t>() : nullptr};
  }
  // The batch list behind the call's last per-sequence kernel on st: waits for the total (the final columns are sized by it),
  // queues the scatter and returns the number of entries.
  int64_t finish(hipStream_t st) {
    const int64_t total = prefix_total(cnt_, n_, off_, st);
    const size_t m = (size_t)total;
    seq_.alloc(4 * m); i_.alloc(4 * m); j_.alloc(4 * m);
    for (int w = 0; w < n_val_; ++w) v_[w].alloc(8 * m);
    if (label_) k_.alloc(4 * m);
    ListCols c{koff_.as<int64_t>(), cnt_.as<int64_t>(), off_.as<int64_t>(), mult_, st_i_.as<int32_t>(), st_j_.as<int32_t>(),
               {st_v_[0].as<double>(), n_val_ > 1 ? st_v_[1].as<double>() : nullptr}, label_ ? st_k_.as<uint8_t>() : nullptr,
               seq_.as<int32_t>(), i_.as<int32_t>(), j_.as<int32_t>(), {v_[0].as<double>(), v_[1].as<double>()}, k_.as<int32_t>()};
    HIP_OK(launch_list_scatter(c, n_, st));
    return count_ = total;
  }
  void set_empty() { count_ = 0; }    // a call that keeps no list
  void invalidate() { count_ = -1; }
  int64_t count() const { return count_; }

  // The list into the caller's columns of cap entries (any may be null).
  void fetch(int32_t* seq, int32_t* i, int32_t* j, double* v0, double* v1, int32_t* k, int64_t cap) const {
    if (count_ < 0) throw StateError(std::string(list_) + " before " + call_);
    if (cap < count_) throw ArgError(std::string(list_) + ": buffer too small");
    const size_t m = (size_t)count_;
    if (m == 0) return;
    fetch_column(seq, seq_, 4 * m); fetch_column(i, i_, 4 * m); fetch_column(j, j_, 4 * m);
    fetch_column(v0, v_[0], 8 * m);
    if (n_val_ > 1) fetch_column(v1, v_[1], 8 * m);
    if (label_) fetch_column(k, k_, 4 * m);
  }

  // The list of a streamed batch on the host: the lists of the chunks' engines one behind the other, with batch-global sequence
  // indices; adopt() makes it the list of the outer handle.
  struct Host {
    std::vector<int32_t> seq, i, j, k;
    std::vector<double> v[2];
    void append(const StagedList& chunk, int c0) {   // c0: the chunk's first sequence
      const size_t b = seq.size(), m = (size_t)std::max<int64_t>(chunk.count_, 0);
      seq.resize(b + m); i.resize(b + m); j.resize(b + m);
      for (int w = 0; w < chunk.n_val_; ++w) v[w].resize(b + m);
      if (chunk.label_) k.resize(b + m);
      chunk.fetch(seq.data() + b, i.data() + b, j.data() + b, v[0].data() + b, chunk.n_val_ > 1 ? v[1].data() + b : nullptr,
                  chunk.label_ ? k.data() + b : nullptr, (int64_t)m);
      for (size_t t = b; t < seq.size(); ++t) seq[t] += c0;
    }
  };
  void adopt(const Host& h, hipStream_t st) {
    seq_.upload(h.seq, st); i_.upload(h.i, st); j_.upload(h.j, st);
    for (int w = 0; w < n_val_; ++w) v_[w].upload(h.v[w], st);
    if (label_) k_.upload(h.k, st);
    HIP_OK(hipStreamSynchronize(st));   // (the host columns go out of use with the copies)
    count_ = (int64_t)h.seq.size();
  }

 private:
  const char* list_; const char* call_;
  int n_val_; bool label_;
  int n_ = 0;
  int64_t mult_ = 1, count_ = -1;
  DevBuf kept_, koff_, cnt_, off_;             // kept cells and their prefix, entries written and their prefix, per batch index
  DevBuf st_i_, st_j_, st_v_[2], st_k_;        // staging
  DevBuf seq_, i_, j_, v_[2], k_;              // the list
};

// The two lists of the loop call, built as a StagedList is: the closing list, (sequence, i, j) and 6 doubles per entry -- p, then the
// LOOP_COLS columns: the layout k_loop_seq and k_loop_scatter write -- and the two-loop list (sequence, i, j, k, l, p).  A closing entry
// is staged at the kept-cell prefix of its sequence, a two-loop entry (item index, T) at the sequence's item_base: a sequence lists at
// most its items.  (Staging by item index: hence no StagedList.)  Counts < 0: no lists (invalidate()).
class LoopLists {
 public:
  // As StagedList::begin, for the n sequences of the resident batch with n_items_total interior-loop items in all: the staging
  // pointers go into la (koff, cnt, cnt2: per batch index; st_*: the closing entries; st2_*: the two-loop entries).
  void begin(const SeqPlan* plans, const uint32_t* okbits, int n, int64_t n_items_total, LoopArgs* la, hipStream_t st) {
    n_ = n;
    kept_.alloc(8 * (size_t)n); koff_.alloc(8 * ((size_t)n + 1)); cnt_.alloc(8 * (size_t)n); cnt2_.alloc(8 * (size_t)n);
    off_.alloc(8 * ((size_t)n + 1)); off2_.alloc(8 * ((size_t)n + 1));
    HIP_OK(launch_pair_kept(plans, okbits, n, kept_.as<int64_t>(), st));
    const size_t cap = (size_t)prefix_total(kept_, n, koff_, st), cap2 = (size_t)std::max<int64_t>(n_items_total, 0);
    st_i_.alloc(4 * cap); st_j_.alloc(4 * cap); st_v_.alloc(8 * kVals * cap); st2_it_.alloc(4 * cap2); st2_t_.alloc(8 * cap2);
    HIP_OK(hipMemsetAsync(cnt_.as<void>(), 0, 8 * (size_t)n, st));
    HIP_OK(hipMemsetAsync(cnt2_.as<void>(), 0, 8 * (size_t)n, st));
    la->koff = koff_.as<int64_t>(); la->cnt = cnt_.as<int64_t>(); la->cnt2 = cnt2_.as<int64_t>();
    la->st_i = st_i_.as<int32_t>(); la->st_j = st_j_.as<int32_t>(); la->st_v = st_v_.as<double>();
    la->st2_it = st2_it_.as<int32_t>(); la->st2_t = st2_t_.as<double>();
  }
  // The batch lists behind the call's last k_loop_seq on st -- by (sequence, i, j), and by outer cell in that order, then in the
  // plan's by-outer order: waits for the two totals and queues the scatter.
  void finish(const SeqPlan* plans, const LoopItem* items, hipStream_t st) {
    const size_t mc = (size_t)prefix_total(cnt_, n_, off_, st), mt = (size_t)prefix_total(cnt2_, n_, off2_, st);
    c_seq_.alloc(4 * mc); c_i_.alloc(4 * mc); c_j_.alloc(4 * mc); c_v_.alloc(8 * kVals * mc);
    t_seq_.alloc(4 * mt); t_i_.alloc(4 * mt); t_j_.alloc(4 * mt); t_k_.alloc(4 * mt); t_l_.alloc(4 * mt); t_p_.alloc(8 * mt);
    LoopListCols lc{plans, items, koff_.as<int64_t>(), cnt_.as<int64_t>(), off_.as<int64_t>(), cnt2_.as<int64_t>(), off2_.as<int64_t>(),
                    st_i_.as<int32_t>(), st_j_.as<int32_t>(), st_v_.as<double>(), st2_it_.as<int32_t>(), st2_t_.as<double>(),
                    c_seq_.as<int32_t>(), c_i_.as<int32_t>(), c_j_.as<int32_t>(), c_v_.as<double>(),
                    t_seq_.as<int32_t>(), t_i_.as<int32_t>(), t_j_.as<int32_t>(), t_k_.as<int32_t>(), t_l_.as<int32_t>(), t_p_.as<double>()};
    HIP_OK(launch_loop_scatter(lc, n_, st));
    n_closing_ = (int64_t)mc; n_two_ = (int64_t)mt;
  }
  void set_empty() { n_closing_ = n_two_ = 0; }    // a call that keeps no lists
  void invalidate() { n_closing_ = n_two_ = -1; }
  int64_t n_closing() const { return n_closing_; }
  int64_t n_two() const { return n_two_; }
  // The lists into the caller's columns of cap entries (any may be null); cols: LOOP_COLS doubles per entry.
  void fetch_closing(int32_t* seq, int32_t* i, int32_t* j, double* p, double* cols, int64_t cap) const {
    if (n_closing_ < 0) throw StateError("loop_closing_list before loop_posteriors");
    if (cap < n_closing_) throw ArgError("loop_closing_list: buffer too small");
    const size_t m = (size_t)n_closing_;
    if (m == 0) return;
    fetch_column(seq, c_seq_, 4 * m); fetch_column(i, c_i_, 4 * m); fetch_column(j, c_j_, 4 * m);
    if (p || cols) {
      std::vector<double> v(kVals * m);
      fetch_column(v.data(), c_v_, 8 * kVals * m);
      for (size_t r = 0; r < m; ++r) {
        if (p) p[r] = v[kVals * r];
        if (cols) for (int k = 0; k < LOOP_COLS; ++k) cols[LOOP_COLS * r + k] = v[kVals * r + 1 + k];
      }
    }
  }
  void fetch_two(int32_t* seq, int32_t* i, int32_t* j, int32_t* k, int32_t* l, double* p, int64_t cap) const {
    if (n_two_ < 0) throw StateError("loop_two_list before loop_posteriors");
    if (cap < n_two_) throw ArgError("loop_two_list: buffer too small");
    const size_t m = (size_t)n_two_;
    if (m == 0) return;
    fetch_column(seq, t_seq_, 4 * m); fetch_column(i, t_i_, 4 * m); fetch_column(j, t_j_, 4 * m);
    fetch_column(k, t_k_, 4 * m); fetch_column(l, t_l_, 4 * m); fetch_column(p, t_p_, 8 * m);
  }
  // The lists of a streamed batch on the host, as StagedList::Host; c_v keeps the 6 doubles per entry.
  struct Host {
    std::vector<int32_t> c_seq, c_i, c_j, t_seq, t_i, t_j, t_k, t_l;
    std::vector<double> c_v, t_p;
    void append(const LoopLists& chunk, int c0) {   // c0: the chunk's first sequence
      const size_t b = c_seq.size(), b2 = t_seq.size();
      const size_t mc = (size_t)std::max<int64_t>(chunk.n_closing_, 0), mt = (size_t)std::max<int64_t>(chunk.n_two_, 0);
      c_seq.resize(b + mc); c_i.resize(b + mc); c_j.resize(b + mc); c_v.resize(kVals * (b + mc));
      t_seq.resize(b2 + mt); t_i.resize(b2 + mt); t_j.resize(b2 + mt); t_k.resize(b2 + mt); t_l.resize(b2 + mt); t_p.resize(b2 + mt);
      chunk.fetch_closing(c_seq.data() + b, c_i.data() + b, c_j.data() + b, nullptr, nullptr, (int64_t)mc);
      if (mc) fetch_column(c_v.data() + kVals * b, chunk.c_v_, 8 * kVals * mc);
      chunk.fetch_two(t_seq.data() + b2, t_i.data() + b2, t_j.data() + b2, t_k.data() + b2, t_l.data() + b2, t_p.data() + b2, (int64_t)mt);
      for (size_t r = b; r < c_seq.size(); ++r) c_seq[r] += c0;
      for (size_t r = b2; r < t_seq.size(); ++r) t_seq[r] += c0;
    }
  };
  void adopt(const Host& h, hipStream_t st) {
    c_seq_.upload(h.c_seq, st); c_i_.upload(h.c_i, st); c_j_.upload(h.c_j, st); c_v_.upload(h.c_v, st);
    t_seq_.upload(h.t_seq, st); t_i_.upload(h.t_i, st); t_j_.upload(h.t_j, st); t_k_.upload(h.t_k, st); t_l_.upload(h.t_l, st); t_p_.upload(h.t_p, st);
    HIP_OK(hipStreamSynchronize(st));   // (the host columns go out of use with the copies)
    n_closing_ = (int64_t)h.c_seq.size(); n_two_ = (int64_t)h.t_seq.size();
  }
 private:
  static constexpr size_t kVals = 1 + LOOP_COLS;   // doubles per closing entry
  int n_ = 0;
  int64_t n_closing_ = -1, n_two_ = -1;
  DevBuf kept_, koff_, cnt_, cnt2_, off_, off2_;         // kept cells and their prefix, entries written and their prefixes, per batch index
  DevBuf st_i_, st_j_, st_v_, st2_it_, st2_t_;           // staging of both lists
  DevBuf c_seq_, c_i_, c_j_, c_v_, t_seq_, t_i_, t_j_, t_k_, t_l_, t_p_;   // the closing list, the two-loop list
};

}  // namespace elemdp
