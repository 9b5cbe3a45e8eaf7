// staged_list.h -- the batch lists of the pair, conditional, stem and helix calls of an Engine (engine.cpp): their buffers and their format.
#pragma once
#include <cstdint>

#include "device_buf.h"
#include "kernels.h"

namespace elemdp {

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
    const size_t cap = (size_t)prefix_total(kept_, koff_, st) * (size_t)mult;
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
    const int64_t total = prefix_total(cnt_, off_, st);
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
    auto get = [&](void* dst, const DevBuf& src, size_t bytes) { if (dst) HIP_OK(hipMemcpy(dst, src.as<void>(), bytes, hipMemcpyDeviceToHost)); };
    get(seq, seq_, 4 * m); get(i, i_, 4 * m); get(j, j_, 4 * m);
    get(v0, v_[0], 8 * m);
    if (n_val_ > 1) get(v1, v_[1], 8 * m);
    if (label_) get(k, k_, 4 * m);
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
  // off[0 .. n_] = exclusive prefix of cnt[0 .. n_), queued on st; waits and returns the total off[n_]
  int64_t prefix_total(const DevBuf& cnt, DevBuf& off, hipStream_t st) {
    HIP_OK(launch_pair_prefix(cnt.as<int64_t>(), n_, off.as<int64_t>(), st));
    int64_t total = 0;
    HIP_OK(hipMemcpyAsync(&total, off.as<int64_t>() + n_, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    return total;
  }

  const char* list_; const char* call_;
  int n_val_; bool label_;
  int n_ = 0;
  int64_t mult_ = 1, count_ = -1;
  DevBuf kept_, koff_, cnt_, off_;             // kept cells and their prefix, entries written and their prefix, per batch index
  DevBuf st_i_, st_j_, st_v_[2], st_k_;        // staging
  DevBuf seq_, i_, j_, v_[2], k_;              // the list
};

}  // namespace elemdp
