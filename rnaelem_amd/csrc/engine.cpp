// engine.cpp -- host side of libelemdp.so: model set-up, batch residency, kernel launches, C ABI.
//
// Mirrors the part of the reference that sits directly around the hot path:
//   RNAelem::set_motif_pattern / set_energy_params      RNAelem/motif_model.hpp:72-97
//   RNAelem::pack_params / unpack_params                 RNAelem/motif_model.hpp:147-168
//   RNAelemTrainer::operator()  (fn / gr assembly)       RNAelem/motif_trainer.hpp:248-271, 595-633
//   RNAelemScanner::scan                                 RNAelem/motif_scanner.hpp:938-949
// There is deliberately no CPU implementation of the DP in this library.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <limits>
#include <memory>
#include <numeric>
#include <random>
#include <sstream>
#include <stdexcept>
#include <string>
#include <mutex>
#include <thread>
#include <vector>

#include <dlfcn.h>

#include "../../include/elemdp.h"
#include "access_rules.h"
#include "automaton.h"
#include "cond_rules.h"
#include "constraint_rules.h"
#include "device_layout.h"
#include "energy_tables.h"
#include "host_prep.h"
#include "kernels.h"
#include "lin_params.h"
#include "live_blocks.h"
#include "node_mea_rules.h"
#include "node_rules.h"
#include "plan_rules.h"
#include "joint_rules.h"
#include "sample_rules.h"
#include "stem_rules.h"
#include "helix_rules.h"
#include "loop_rules.h"
#include "staged_list.h"
#include "structure_rules.h"
#include "table_slots.h"

namespace elemdp {
namespace {

thread_local std::string g_error;
std::string g_data_dir;

// Makes `device` the calling thread's current HIP device for the lifetime of the guard and restores the previous one.  Every
// computing entry point of an Engine takes one: the current device is a per-thread setting, so a handle used from another
// host thread (the prefetch thread of the mini-batch loop), or a second handle on another GPU, must not inherit whatever
// device was current.
class DeviceGuard {
 public:
  explicit DeviceGuard(int device) {
    if (device < 0) return;
    if (hipGetDevice(&prev_) != hipSuccess) prev_ = -1;
    if (prev_ != device) { HIP_OK(hipSetDevice(device)); changed_ = true; }
  }
  ~DeviceGuard() { if (changed_ && prev_ >= 0) (void)hipSetDevice(prev_); }
  DeviceGuard(const DeviceGuard&) = delete;
  DeviceGuard& operator=(const DeviceGuard&) = delete;

 private:
  int prev_ = -1;
  bool changed_ = false;
};

// RCCL entry points, resolved at run time: the library has no link-time dependency on librccl (hosts that bring their own
// collective -- torch.distributed in rnaelem_amd/distributed.py -- never load it)
struct Rccl {
  typedef struct { char internal[128]; } UniqueId;           // ncclUniqueId (rccl.h: NCCL_UNIQUE_ID_BYTES = 128)
  typedef void* Comm;                                         // ncclComm_t
  int (*GetUniqueId)(UniqueId*) = nullptr;
  int (*CommInitRank)(Comm*, int, UniqueId, int) = nullptr;
  int (*AllReduce)(const void*, void*, size_t, int, int, Comm, hipStream_t) = nullptr;
  int (*CommDestroy)(Comm) = nullptr;
  const char* (*GetErrorString)(int) = nullptr;
  static constexpr int kDouble = 8, kSum = 0;                 // ncclFloat64, ncclSum
  static Rccl& get() {
    static Rccl r;
    static std::once_flag once;   // (engines are driven from two host threads when a batch is streamed)
    std::call_once(once, [] {
      void* lib = nullptr;
      for (const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"})
        if ((lib = dlopen(name, RTLD_NOW | RTLD_LOCAL))) break;
      if (lib) {
        r.GetUniqueId = reinterpret_cast<decltype(r.GetUniqueId)>(dlsym(lib, "ncclGetUniqueId"));
        r.CommInitRank = reinterpret_cast<decltype(r.CommInitRank)>(dlsym(lib, "ncclCommInitRank"));
        r.AllReduce = reinterpret_cast<decltype(r.AllReduce)>(dlsym(lib, "ncclAllReduce"));
        r.CommDestroy = reinterpret_cast<decltype(r.CommDestroy)>(dlsym(lib, "ncclCommDestroy"));
        r.GetErrorString = reinterpret_cast<decltype(r.GetErrorString)>(dlsym(lib, "ncclGetErrorString"));
      }
    });
    return r;
  }
  bool ok() const { return GetUniqueId && CommInitRank && AllReduce && CommDestroy; }
};
#define RCCL_OK(expr)                                                                                                     \
  do {                                                                                                                    \
    int r_ = (expr);                                                                                                      \
    if (r_ != 0)                                                                                                          \
      throw elemdp::HipError(std::string(#expr) + ": " +                                                                  \
                             (elemdp::Rccl::get().GetErrorString ? elemdp::Rccl::get().GetErrorString(r_) : "rccl error")); \
  } while (0)

// sets a variable for a scope: the old value comes back however the scope is left
template <class T> class ScopedValue {
 public:
  ScopedValue(T& ref, T v) : ref_(ref), old_(ref) { ref_ = v; }
  ~ScopedValue() { ref_ = old_; }
  ScopedValue(const ScopedValue&) = delete;
  ScopedValue& operator=(const ScopedValue&) = delete;

 private:
  T& ref_;
  T old_;
};

std::string default_data_dir() {
  if (!g_data_dir.empty()) return g_data_dir;
  if (const char* e = std::getenv("ELEMDP_DATA_DIR")) return e;
  Dl_info info;
  if (dladdr(reinterpret_cast<void*>(&default_data_dir), &info) && info.dli_fname) {
    std::string p(info.dli_fname);
    size_t k = p.find_last_of('/');
    return (k == std::string::npos ? std::string(".") : p.substr(0, k)) + "/data";
  }
  return "data";
}

std::string read_file(const std::string& path) {
  std::ifstream f(path);
  if (!f) throw ArgError("cannot open energy parameter file: " + path);
  std::stringstream ss;
  ss << f.rdbuf();
  return ss.str();
}

// one set of plan arrays (for a subset of the batch)
struct PlanSet {
  int first = 0, count = 0;
  std::vector<SeqPlan> h;
  DevBuf d_plans, dmin, e_stack, e_ext, e_ml, e_close, e_hp, off_outer, off_inner, off_left, off_right, cursor, items,
      item_in, idx_inner, idx_left, idx_right, items_inner, items_left, items_right;
  // usefulness mask of the train sweeps (PlanArrays::useful), built by the first train evaluation that wants it
  // (Engine::ensure_useful_mask): a batch that is only scanned never pays for it
  DevBuf useful;
  bool useful_built = false;
  // pair terms of the outside train sweep (PlanArrays::ha_rows / h1_stems), built right behind the mask, once per plan; not where
  // the plan gets no words: W > 64, or the mask of all ones
  DevBuf pair_words;
  bool pair_terms_built = false;
  // live-block lists of the train sweeps (PlanArrays::blocks; Engine::ensure_live_blocks) for `blk_cpb` cells per block that span
  // at most `blk_cap` cells, and the largest block count of every diagonal over the set (host copy: the grids)
  DevBuf blocks, blk_max;
  int64_t n_blocks = 0;
  int blk_cpb = 0, blk_cap = 0;
  std::vector<int32_t> h_blk_max, h_blk_grid;
  std::vector<int32_t> h_blk_grid_in;   // the same choice for the inside set (the lists of the bytes without UB_L: live_blocks.h)
  bool blk_all = false;            // built under live_blocks 2 (lists on every diagonal)
  bool blk_two = false;            // the inside set (the bytes without UB_L) is built too: only where the loop pre-pass runs, or for its read-back
  int64_t n_cells = 0;
  bool permuted = false;   // keep item copies in the secondary orders (resident plan of the train pipeline)
  bool inner_only = false; // build only the by_inner order (the BPP filter needs no outside values of loop cells)
  bool sorted = true;      // the segments of the role lists are sorted by item index (Engine::ensure_sorted_plan)
  PlanKernelArgs ka;       // the arguments the set was built with (for the sort, should a later evaluation want it)
  int64_t n_items = 0;
  PlanArrays arrays() const {
    PlanArrays a;
    a.dmin = dmin.as<int16_t>();
    a.e_stack = e_stack.as<double>(); a.e_ext = e_ext.as<double>(); a.e_ml = e_ml.as<double>();
    a.e_close = e_close.as<double>(); a.e_hp = e_hp.as<double>();
    a.by_outer_off = off_outer.as<int32_t>(); a.by_inner_off = off_inner.as<int32_t>();
    a.by_left_off = off_left.as<int32_t>(); a.by_right_off = off_right.as<int32_t>();
    a.cursor = cursor.as<int32_t>();
    a.items = items.as<LoopItem>(); a.item_in = item_in.as<uint8_t>();
    a.by_inner_idx = idx_inner.as<int32_t>(); a.by_left_idx = idx_left.as<int32_t>(); a.by_right_idx = idx_right.as<int32_t>();
    a.items_inner = items_inner.as<LoopItem>(); a.items_left = items_left.as<LoopItem>(); a.items_right = items_right.as<LoopItem>();
    return a;
  }
};

}  // namespace

class Engine {
 public:
  explicit Engine(const elemdp_model_desc& d);
  ~Engine();

  void useful_mask(int idx, uint8_t* mask, int cap);
  void pair_terms(int idx, uint64_t* ha, uint64_t* h1, int cap);
  void live_blocks(int idx, int32_t* counts, void* records, int stride, int32_t* cpb_cap, int32_t* taken, bool inside = false);
  int n_param() const { return au_.n_theta() + 2; }
  int n_state() const { return au_.S(); }
  int n_node() const { return au_.M(); }
  const Automaton& automaton() const { return au_; }
  const AutomatonLayout& layout() const { return lays_.shadow >= 0 ? lays_ : lay_; }   // (what a train evaluation sweeps)
  bool softmax() const { return flags_ & ELEMDP_THETA_SOFTMAX; }

  void load_batch(const uint8_t* seq, const int32_t* off, const uint8_t* qual, const int32_t* qoff, const char* fix, int n,
                  const char* cons = nullptr);
  // reduce: all-reduce the vector over the communicator of elemdp_comm_init (if any) before it is handed out
  void train_partial(const double* x, int n_param, void* partial, bool device_ptr, bool reduce = false);
  void train_finish(const double* reduced, double* fn, double* gr, double* sum_eff, int32_t* n_skipped);
  void scan(const double* x, int n_param, elemdp_scan_out* out);
  // base-pair posteriors of the batch under the motif model (pair_rules.h); the list stays on the device for pair_list
  // mea (optional): also the maximum expected accuracy structures over the same P (mea_rules.h)
  struct MeaOut { double gamma; char* structure; double* score; };
  void pair_posteriors(const double* x, int n_param, double min_prob, int64_t* n_pairs, double* unpaired, const MeaOut* mea = nullptr);
  void pair_list(int32_t* seq, int32_t* i, int32_t* j, double* p, int64_t cap);
  // motif-conditional pair posteriors (cond_rules.h): the fold with the motif and the fold without it; outputs as
  // elemdp_pair_conditional, any may be null; gamma is read only where a structure is asked for.  The list stays on the device
  // for cond_list; the list of the last pair_posteriors is left alone.
  struct CondOut { double gamma; double* exist; double* unpaired[2]; char* structure[2]; double* shift; };
  void pair_conditional(const double* x, int n_param, double min_prob, int64_t* n_pairs, const CondOut& out);
  void cond_list(int32_t* seq, int32_t* i, int32_t* j, double* p_motif, double* p_none, int64_t cap);
  // stochastic samples of derivations (sample_rules.h); outputs as elemdp_sample
  struct SampleOut { char* rss; uint8_t* node; double* logp; int32_t* status; };
  void sample_structures(const double* x, int n_param, int n_samples, uint64_t seed, int64_t index_base, const SampleOut& out);
  // structural context profiles (ctx_rules.h): 7 doubles per position of the batch, O L R H B I M
  void context_profile(const double* x, int n_param, double* profile);
  // posterior motif-node profiles (node_rules.h): n_node doubles per position of the batch
  void node_profile(const double* x, int n_param, double* profile);
  // joint node-by-context posteriors (joint_rules.h): 35 n_node counts per sequence, and on request 7 n_node
  // doubles per position of the batch
  void joint_profile(const double* x, int n_param, double* counts, double* profile);
  // pair posteriors by motif node pair (stem_rules.h): 25 K counts per sequence; with a finite min_prob the
  // labelled list stays on the device for stem_list.  stem_slots: the node pair of every slot (host only), returns K.
  int stem_slots(int32_t* node_left, int32_t* node_right, int cap) const;
  void stem_profile(const double* x, int n_param, double min_prob, double* counts, int64_t* n_entries);
  void stem_list(int32_t* seq, int32_t* i, int32_t* j, int32_t* slot, double* q, int64_t cap);
  // helix posteriors (helix_rules.h): the joint probability of every run of min_len .. max_len stacked pairs that
  // reaches min_prob; with a finite min_prob the list stays on the device for helix_list.  structure: dot-bracket strings in seq_off
  // indexing or null; stem_len / stem_prob (seq_off indexing, either may be null): at the 5' base of the outermost pair of every
  // stem of the structure its length and the joint probability of the whole stem, 0 / NaN elsewhere.
  void helix_posteriors(const double* x, int n_param, int max_len, int min_len, double min_prob, int64_t* n_entries,
                        const char* structure, int32_t* stem_len, double* stem_prob);
  void helix_list(int32_t* seq, int32_t* i, int32_t* j, int32_t* len, double* p, int64_t cap);
  // loop posteriors (loop_rules.h): what every pair closes (H S B I M) and the two-loops; with a finite min_prob the
  // two lists stay on the device for loop_closing_list / loop_two_list.  counts (5 per sequence) may be null.  structure: dot-bracket
  // strings in seq_off indexing or null; loop_type / loop_prob (seq_off indexing, either may be null): at the 5' base of every pair
  // of the structure the type of the loop it closes and the loop's probability, 0 / NaN elsewhere.
  void loop_posteriors(const double* x, int n_param, double min_prob, double* counts, int64_t* n_closing, int64_t* n_two,
                       const char* structure, int32_t* loop_type, double* loop_prob);
  void loop_closing_list(int32_t* seq, int32_t* i, int32_t* j, double* p, double* cols, int64_t cap);
  void loop_two_list(int32_t* seq, int32_t* i, int32_t* j, int32_t* k, int32_t* l, double* p, int64_t cap);
  // accessibility (access_rules.h): max_width doubles per position of the batch, the widths 1 .. max_width
  void accessibility(const double* x, int n_param, int max_width, double* access);
  // maximum expected accuracy motif alignments and site lists over that profile (node_mea_rules.h); outputs as
  // elemdp_node_mea, any may be null
  struct NodeMeaOut { double* profile; uint8_t* node; int32_t* n_sites; int32_t* start; int32_t* end; double* score; double* conf; };
  void node_mea(const double* x, int n_param, double gamma, int max_sites, const NodeMeaOut& out);
  int partial_len() const { return 4 + 2 * au_.n_theta() + 4; }
  void set_option(const std::string& key, double v);
  void comm_init(int rank, int world, const void* id);
  void comm_destroy();
  bool has_comm() const { return comm_ != nullptr; }

  int n_seq() const { return n_seq_; }
  const std::vector<SeqPlan>& plans() const { return h_plans_; }
  void seq_stats(double* out, int n);
  void seq_counts(double* out, int n);
  bool bpp_eff_known() const {
    if (!streaming_) return true;
    for (char c : st_have_eff_) if (!c) return false;
    return true;
  }
  void debug_tables(double* inside, double* outside, double* inside_o, double* outside_o, double* ENo, double* ENx, double* EH);
  void batch_pairs(int idx, uint8_t* kept, double* lnbpp, int cap);
  double last_ms[3] = {0, 0, 0};
  // the last train evaluation ran with the zeros of the dead entries kept in the slots (TableSlots::zeros), and the slots the
  // handle holds: elemdp_last_timing entries 3 and 4
  bool last_zeros_kept() const { return last_zeros_kept_; }
  int slots_held() const { return slots_.n_held(); }
  // options recorded for the inner engines of a streamed batch (elemdp_last_timing entry 5: setting "world" around every call adds none)
  int options_logged() const { return (int)opt_log_.size(); }

 private:
  void upload_params(const double* x, const AutomatonLayout& lay, bool trivial);
 public:
  void set_theta_from(const double* x);  // host: theta (log-softmax of x when theta-softmax)
 private:
  // ---- the stages of load_batch
  struct BatchShape {   // a checked batch: the records' plans (L, W, C, positive, offsets into the batch arrays), its extent
    std::vector<SeqPlan> plans;
    int Lmax = 0, Wmax = 0, nword_max = 0;
    int64_t n_bases = 0, n_pos = 0, n_words = 0, n_cells = 0;
  };
  BatchShape check_batch(const uint8_t* seq, const int32_t* off, const uint8_t* qual, const int32_t* qoff, const char* fix, int n) const;
  void stage_batch(BatchShape&& b, const uint8_t* seq, const int32_t* off, const uint8_t* qual, const int32_t* qoff, const char* fix,
                   std::vector<uint8_t>& h_seq, std::vector<uint32_t>& fix_bits);
  const uint32_t* bpp_filter(const std::vector<uint32_t>& fix_bits);
  // hard constraints: the rows of the strings, checked on the host; the mask, unp and ndot of the constrained batch
  struct ConsRows { std::vector<uint8_t> cls, unp; std::vector<int32_t> partner, enc, ndot; };
  ConsRows constraint_rows(const BatchShape& b, const uint8_t* seq, const int32_t* off, const char* cons, bool check_only) const;
  const uint32_t* constrain(const uint32_t* mask, const ConsRows& rows);
  void bpp_chunks(bool lin);
  void bpp_lin_chunk(int first, int count, int64_t cells, double* lnbpp);
  void bpp_log_chunk(int first, int count, int64_t cells, double* lnbpp);
  void resident_plan(const uint32_t* mask);
  void build_planset(PlanSet& ps, int first, int count, const uint32_t* d_okbits);
  void ensure_sorted_plan();
  void ensure_useful_mask();
  bool ensure_live_blocks(int cpb, int cap, bool inside_too);
  bool loop_prepass_ok(bool sched1) const;
  bool loop_outside_ok(bool sched1) const;
  int live_span_for(int cpb) const;
  bool lists_wanted() const;
  LdsLayout lds_layout(const AutomatonLayout& lay, int Lmax, int nword_max, bool scan) const;
  DpArgs base_args(const AutomatonLayout& lay, const int32_t* d_ints, const double* d_params, const PlanSet& ps,
                   const uint32_t* d_okbits, int S);
  // the request for table slots of the loaded batch under the handle's options (its fields: slot_sizing.h)
  SlotRequest slot_request(int S, int row, bool scan, int n_want, int group = 0, int pair_row = 0) const;
  void run_train();
  void run_train_batch();
  void run_lin_batch();
  // group_cap: most sequences swept in lockstep (a scan uses fewer: fresh table memory costs ~20 ms / GB)
  // own: the call may give every sequence a slot of its own (option own_slots; decided here: own_map_)
  int prepare_lin(LinArgs& a, bool sched1, bool dense_too = false, int n_eval = 0, int group_cap = 8192, bool own = false);
  ZeroBinding zero_binding(const LinArgs& a, bool sched1, bool ranged) const;
  template <class Work> void sweep_groups(const LinArgs& a, int n, const int32_t* h_ord, const int32_t* d_ord, const SeqPlan* d_sorted,
                                          int gsz, int ns, Work work);
  struct ScanPos {   // what a scan's first sum pass writes besides its tables: per position, then per sequence
    DevBuf start, inner, end, ys, ye, exist;
    ScanPos(size_t n_seqpos, int n) {
      start.alloc(8 * n_seqpos); inner.alloc(8 * n_seqpos); end.alloc(8 * (n_seqpos + n));
      ys.alloc(4 * (size_t)n); ye.alloc(4 * (size_t)n); exist.alloc(8 * (size_t)n);
    }
  };
  int prepare_scan(LinArgs& a, const ScanPos& pos);
  int read_flagged(std::vector<int32_t>* list = nullptr);
  DpArgs log_scan_args(bool sums_on_batch, int* n_blocks);
  int log_chunk(int n_blocks, int n_log) const;
  template <class T> T* slot_scratch(DevBuf& b, size_t stride, size_t slot0 = 0);
  PairArgs pair_batch_args() const;
  void pair_plane_fields(PairArgs& pa, const LinArgs& a) const;
  void require_resident(const char* what, int n_param_in);
  template <class Fill, class Group> int scan_sums(const ScanPos& pos, Fill fill, Group group, std::vector<int32_t>* flagged = nullptr);
  template <class Fill, class Behind> void scan_log_form(bool sums_on_batch, int n_flagged, Fill fill, Behind behind);
  template <class Fill, class Group, class LogFill, class Behind>
  int scan_both_forms(const ScanPos& pos, Fill fill, Group group, LogFill log_fill, Behind behind, bool in_world = true);
  void finish_call(int n_flagged);
  template <class Copy> void finish_call(int n_flagged, Copy copy_out);
  int node_profile_device(const char* what, const double* x, int n_param_in);
  TrArgs log_pipeline_args();
  void init_device();
  void flatten_automaton();
  bool poison_tables();
  void lin_weights(int first = 0, int count = 0);
  void upload_automaton();
  bool opt_prune_ = true;   // transition lists pruned to the transitions of complete parses (Automaton::flatten)
  // a train evaluation covers the records [eval_first, eval_first + eval_count) of the resident batch only (count 0: all): the
  // mini-batch trainer loads the records + negatives of several coming evaluations as ONE batch -- the filter and the plan do not
  // depend on x, and a load of 128 sequences costs as much as one of 1024 (launch-bound) -- and evaluates them range by range
  int opt_eval_first_ = 0, opt_eval_count_ = 0;
  std::vector<int32_t> h_order_r_;
  DevBuf d_order_r_, d_plans_sorted_r_;
  int range_key_[2] = {-1, -1};
  bool opt_det_ = false;    // deterministic reductions of the scaled-linear train evaluation (LinArgs::det): bit-identical repeats
  bool opt_fast_ = true;    // table-driven unary phases of the train kernels (lin_fast.h); 0 = the generic rule code
  bool opt_own_slots_ = true;   // option "own_slots": an unranged train evaluation of a resident batch gives every sequence a slot of
                                // its own where the batch fits (slot_sizing.h), and the zeros of dead entries stay from one evaluation
                                // to the next; 0: the slots of one group, shared by the groups of a stream
  bool own_map_ = false;        // the mapping of the last prepare_lin: a slot per sequence, groups cut for lock_slots_ slots
  int lock_slots_ = 0;
  bool last_zeros_kept_ = false;
  unsigned long long plan_gen_ = 0;   // identity of plan_, its mask and its lists (ZeroBinding::plan)
  int opt_world_ = 0;       // 0 mixture, 1 motif, 2 none: the world of the scan family's posterior products
  bool opt_poison_ = false; // tests: the table slots are filled with NaN before every evaluation of the scaled-linear pipeline, so
                            // that a read of an entry nobody stored shows up in the results (the compact tables hold garbage there)
  void require_device() const;
  bool has_device_ = false;
  int want_device_ = -1;
  Rccl::Comm comm_ = nullptr;   // in-library collective (elemdp_comm_init): all-reduce of the partial vector in train_eval
  int comm_rank_ = 0, comm_world_ = 1;
  // ---- streaming: a batch that is not kept resident as a whole (option "max_resident", or more sequences than the device
  // memory holds).  The handle then keeps the host copy of the input and two inner engines on the same device: chunk k is
  // evaluated (or scanned) on one while the other runs load_batch (BPP filter + plan) of chunk k+1 on a second host thread;
  // the partial vectors of the chunks are summed in chunk order.  The reference streams its records the same way
  // (motif_trainer.hpp:124-153 over fastq_io.hpp:132-167) and recomputes the BPP filter in every evaluation, too.
  bool streaming_ = false;
  int st_chunk_ = 0, opt_max_resident_ = 0;
  // an inner handle of a streamed batch: never streams itself, and its table slots stay inside the share of the device
  // memory the outer handle left for them (two inner handles: plan + slots of each within 2/5 of the free memory)
  bool inner_ = false;
  size_t slot_budget_ = 0, st_slot_budget_ = 0;
  std::vector<uint8_t> st_seq_, st_qual_;
  std::vector<char> st_fix_, st_cons_;
  std::vector<double> st_rows_;                             // [Z(ari,nasi), Z(ari), Z(nasi), f, skipped] per sequence
  std::unique_ptr<Engine> sub_[2];
  std::vector<std::pair<std::string, double>> opt_log_;     // options to replay on the inner engines
  elemdp_model_desc desc_;
  std::string desc_pattern_, desc_par_;
  bool desc_has_par_ = false;
  bool should_stream(const BatchShape& b);
  void stream_setup(const uint8_t* seq, const int32_t* off, const uint8_t* qual, const int32_t* qoff, const char* fix,
                    BatchShape&& b);
  void stream_load_chunk(int k, Engine& e);
  // The BPP filter does not depend on the parameters: a streamed batch keeps the filtered pair mask (1.3 KB per sequence of
  // L = 200) and the kept fractions of every chunk on the host after its first load; later loads of the chunk hand them
  // to the inner handle, which then skips K1 and only rebuilds the plan.
  std::vector<std::vector<uint32_t>> st_mask_;
  std::vector<std::vector<double>> st_eff_;
  std::vector<char> st_have_eff_;        // chunk k has been loaded at least once: its bpp_eff values are known
  const uint32_t* preset_bits_ = nullptr;   // (consumed by the next load_batch)
  const double* preset_eff_ = nullptr;
  size_t preset_words_ = 0;
  size_t bits_words_ = 0;                   // words of the pair mask of the loaded batch
  void set_filter_preset(const uint32_t* bits, size_t words, const double* eff) { preset_bits_ = bits; preset_words_ = words; preset_eff_ = eff; }
  void filter_result(std::vector<uint32_t>& bits, std::vector<double>& eff) {
    bits.resize(bits_words_);
    // (of a constrained batch the mask from before k_constrain: the cache holds the filter's result)
    HIP_OK(hipMemcpyAsync(bits.data(), (constrained_ && d_okbits_f_.bytes()) ? d_okbits_f_.as<void>() : d_okbits1_.as<void>(), sizeof(uint32_t) * bits_words_,
                          hipMemcpyDeviceToHost, st_));
    HIP_OK(hipStreamSynchronize(st_));
    eff.resize(h_plans_.size());
    for (size_t k = 0; k < h_plans_.size(); ++k) eff[k] = h_plans_[k].bpp_eff;
  }
  void stream_subs();
  template <class Checked, class Work> void stream_call(int n_param_in, Checked checked, Work work);
  void stream_train(const double* x, int n_param, void* partial, bool device_ptr, bool reduce);
  void stream_scan(const double* x, int n_param, elemdp_scan_out* out);
  void stream_pairs(const double* x, int n_param, double min_prob, double* unpaired, const MeaOut* mea);
  void stream_samples(const double* x, int n_param, int n_samples, uint64_t seed, int64_t index_base, const SampleOut& out);
  void stream_cond(const double* x, int n_param, double min_prob, const CondOut& out);
  template <class List, class ChunkCall> void stream_listed(List Engine::*list, int n_param_in, ChunkCall call);
  // the lists of the last pair, conditional, stem, helix and loop call (staged_list.h), each in buffers of its own
  StagedList pairs_{"pair_list", "pair_posteriors", 1, false};
  StagedList conds_{"pair_conditional_list", "pair_conditional", 2, false};
  StagedList stems_{"stem_list", "stem_profile", 1, true};
  StagedList helices_{"helix_list", "helix_posteriors", 1, true};
  LoopLists loops_;
  size_t scratch_slots_ = 0;   // slots the per-slot scratch of the running scan-family call is sized for (slot_scratch)
  DevBuf d_pr_P_, d_pr_unp_;   // pair posteriors: the P(i, d) scratch of the table slots, the unpaired vector of the call
  // MEA structures: the M table and choice scratch of the table slots (as d_pr_P_), the structures and the scores of the call
  DevBuf d_mea_M_, d_mea_ch_, d_mea_s_, d_mea_sc_;
  DevBuf d_sm_rss_, d_sm_node_, d_sm_logp_, d_sm_status_, d_sm_stack_;   // sample_structures
  // conditional pair posteriors, all of the call's own: the P(i, d) scratch of both worlds per table slot, ln Z per slot of the
  // log-space form, unpaired vectors, exist_prob and shift, then the MEA scratch, structures and scores of both worlds
  DevBuf d_cd_P_[2], d_cd_z_, d_cd_unp_[2], d_cd_exist_, d_cd_shift_;
  DevBuf d_cd_M_, d_cd_ch_, d_cd_s_[2], d_cd_sc_;
  // context profiles: P, u, h, b of the table slots (four [i][d] arrays per slot), their exterior columns, the profile of the call
  DevBuf d_cx_cells_, d_cx_o_, d_cx_prof_;
  DevBuf d_ac_T_, d_ac_vec_, d_ac_out_;   // accessibility: the four planes per slot, the log-space form's vectors, the result
  DevBuf d_jn_lists_, d_jn_X_, d_jn_vec_, d_jn_prof_, d_jn_counts_;   // joint profiles: lists and slot map, per-cell scratch per slot, the log-space form's vectors, the results
  // stem profiles: the transitions by slot, Q of the table slots, the parse marks and counts of the call
  DevBuf d_sp_lists_, d_sp_X_, d_sp_has_, d_sp_counts_;
  // helix posteriors: P, the units (count, i, d, reached length) and their values per table slot, the log-space form's vectors, the
  // stems of the caller's structures (offsets per sequence, i, d, length) and their probabilities
  DevBuf d_hx_P_, d_hx_nu_, d_hx_ui_, d_hx_ud_, d_hx_nlen_, d_hx_X_, d_hx_vec_;
  DevBuf d_hx_soff_, d_hx_si_, d_hx_sd_, d_hx_slen_, d_hx_sp_;
  // loop posteriors: P, the units (count, i, d), their columns and the two-loop values per table slot; the counts of the call; the
  // loops of the caller's structures (offsets per sequence, type, i, d, k, l) and their probabilities.  (The lists: loops_.)
  DevBuf d_lp_P_, d_lp_nu_, d_lp_ui_, d_lp_ud_, d_lp_cols_, d_lp_T_, d_lp_counts_;
  DevBuf d_lp_soff_, d_lp_st_, d_lp_si_, d_lp_sd_, d_lp_sk_, d_lp_sl_, d_lp_sp_;
  DevBuf d_nd_lists_, d_nd_prof_;   // node profiles: the transitions by emitted node, the profile of the call
  // node MEA: the chain lists, the backpointer scratch (M bytes per position), the rows, sites per sequence, start / end / score / confidence per slot
  DevBuf d_nm_lists_, d_nm_bp_, d_nm_node_, d_nm_ns_, d_nm_s0_, d_nm_s1_, d_nm_sc_, d_nm_cf_;

  Automaton au_;
  EnergyTables et_;
  AutomatonLayout lay_, lay0_, layr_;
  std::vector<int32_t> ints_, ints0_, intsr_;
  bool linear_ok_ = true;
  int flags_, max_span_, max_iloop_;
  bool loops_finite_ = false;   // loop_tables_finite(et_)
  double min_bpp_, tau_;
  // shortest hairpin: m_min of the DP rules, min_span of the pair masks (ELEMDP_DBG_NO_TURN drops the turn)
  int m_min() const { return (flags_ & ELEMDP_DBG_NO_TURN) ? 4 : 10; }
  int min_span() const { return (flags_ & ELEMDP_DBG_NO_TURN) ? 1 : 5; }
  int device_ = -1, n_cu_ = 256;   // device_ < 0: no HIP device (host-only handle)
  hipStream_t st_ = nullptr;
  hipEvent_t ev_[4] = {nullptr, nullptr, nullptr, nullptr};
  // groups evaluated concurrently (sweep_groups): stream k of gs_ (gs_[0] = st_)
  static constexpr int kMaxGroupStreams = 4;
  hipStream_t gs_[kMaxGroupStreams] = {nullptr, nullptr, nullptr, nullptr};
  // (created when first used: the runtime deals its few hardware queues to streams in the order they are made, and two
  // handles that evaluate and load at the same time -- the mini-batch trainer -- must not end up sharing one)
  void need_group_streams(int ns) {
    for (int k = 1; k < ns && k < kMaxGroupStreams; ++k)
      if (!gs_[k]) HIP_OK(hipStreamCreateWithFlags(&gs_[k], hipStreamNonBlocking));
  }
  hipEvent_t gdone_[kMaxGroupStreams] = {}, gstart_ = nullptr;
  int opt_group_streams_ = 2;
  // streams for a sweep whose schedule allows concurrent groups
  int group_streams(bool concurrent) const {
    return (concurrent && opt_group_streams_ >= 2) ? std::min(opt_group_streams_, kMaxGroupStreams) : 1;
  }
  DevBuf d_et_, d_xet_, d_ints_, d_ints0_, d_params_, d_params0_, d_counter_, d_lay_, d_lay0_, d_layr_, d_intsr_;
  std::vector<double> theta_;  // log-probabilities of the last evaluation (softmax Jacobian)

  // batch
  int n_seq_ = 0, Lmax_ = 0, Wmax_ = 0, nword_max_ = 0;
  std::vector<SeqPlan> h_plans_;
  std::vector<int32_t> h_order_, h_seq_off_, h_qual_off_;
  DevBuf d_seq_, d_ws_, d_unp_, d_ndot_, d_okbits0_, d_okbits1_, d_order_, d_ncanon_;
  // a constrained batch (elemdp_load_batch_constrained): set behind the BPP filter, which sees no constraint.  The rows of the
  // strings, and the filter's mask from before k_constrain (a streamed batch caches that one)
  bool constrained_ = false;
  DevBuf d_cons_cls_, d_cons_partner_, d_cons_enc_, d_okbits_f_;
  std::vector<double> h_lnbpp_;          // optional (keep_lnbpp)
  std::vector<int64_t> h_lnbpp_base_;
  PlanSet plan_;
  TableSlots slots_;
  DevBuf d_seq_out_, d_partial_;
  int out_stride_ = 0;
  // options
  int opt_slots_ = 0;
  bool opt_keep_lnbpp_ = false;
  bool opt_first_pass_only_ = false;
  bool opt_profile_ = false;
  // 4 = scaled-linear batch pipeline (lin_kernels.hip), 3 = log-space batch pipeline, 2 = fused one-workgroup-per-sequence kernel
  int opt_pipeline_ = 4;
  bool opt_useful_mask_ = true;    // option "useful_mask": the train sweeps skip the entries no complete parse reaches
  bool opt_pair_terms_ = true;     // option "pair_terms": the pair sums of the outside train sweep walk the plan's words of useful rows and stems
  int opt_live_blocks_ = 1;        // option "live_blocks": a workgroup of the train sweeps takes cpb LIVE cells of its diagonal;
                                   // 2: on every diagonal, also where the lists save no workgroups
  int opt_live_span_ = 0;          // option "live_span": the cells a block may span (0: kLiveSpanDefault, at least cpb)
  bool opt_loop_prepass_ = true;   // option "loop_prepass": a row pre-pass fills the inside L plane of the table-driven train sweep, whose
                                   // workgroups then skip the cells that are useful in L alone; 0 = the sweep computes L itself
  bool opt_loop_outside_ = true;   // option "loop_outside": the outside L plane (heavy sum HL, chain, 6b statistic, chain counts) is made by
                                   // two kernels behind the table-driven train sweep, which skips the cells that are useful in L alone
                                   // (DESIGN §4.6); ignored in the deterministic mode; 0 = the sweep computes L itself
  int opt_useful_lds_kb_ = 150;    // option "useful_mask_lds_kb": k_useful_mask's LDS budget; a larger sequence gets the all-ones mask
  bool opt_sorted_plan_ = false;   // option "sorted_plan": sort the role lists at load_batch whatever the pipeline
  // scaled-linear pipeline
  AutomatonLayout lays_;                 // the automaton with the shadow copy of (0,0): both outside passes in one sweep
  std::vector<int32_t> intss_;
  DevBuf d_lays_, d_intss_;
  std::vector<double> last_x_;           // parameters of the last train evaluation (debug_tables repeats it with the generic kernels)
  std::vector<double> h_lin_, h_lins_;   // linear parameter block of the last evaluation (plain automaton / with the shadow state)
  std::vector<uint8_t> h_seq_;           // base codes of the batch (table export)
  HostBuf hb_ws_, hb_ews_, hb_unp_;      // staging of load_batch
  int64_t n_cells_total_ = 0;
  bool train_rows_ = false;              // d_seq_out_ holds the rows of a train evaluation (seq_counts)
  int n_flagged_last_ = 0;
  DevBuf d_plans_sorted_;   // plan records in processing (h_order_) order
  DevBuf d_ews_, d_xwc_, d_xwi_, d_lin_, d_lins_, d_flagged_, d_det_;
  int opt_schedule_ = 1;   // 1 = linear (ari pass + one-state nasi pass), 0 = the reference's two full passes
  int opt_dbg_ = 0;        // timing experiments (LinArgs::dbg); results are wrong when set
  int opt_group_ = 0;      // sequences swept in lockstep by the batch pipeline (0 = auto)
  int opt_access_terms_ = 15;     // accessibility: the terms that take part (bit AccessTerm)
  int opt_node_rules_ = NR_ALL;   // node_profile: the emitting rules that take part (NodeRule bits)
  DevBuf d_prof_;
  DevBuf d_okbits_end_, d_nitems_, d_plans_all_;   // scratch of build_planset and of the canonical mask, kept across loads
  // scratch of the BPP filter, which nothing else reads; kept across loads (the mini-batch trainer loads before every evaluation)
  struct BppScratch {
    DevBuf band_in, band_out, ext_in, ext_out, tmp;   // planes of the linear form / S = 1 table slots of the log-space form
    DevBuf kept;                                      // pairs kept per sequence of the chunk
    DevBuf plans, xw, dmin, cand, plist, poff;        // linear form (bpp_kernels.hip)
    bool planes_finite = false;                       // ... its planes hold nothing but finite values (cleared at allocation)
    PlanSet plan;                                     // log-space form: plan over the unfiltered mask, chunk by chunk
    DevBuf order, rows, zero_ws;                      // ... its sweep order, output rows and weights (all 0)
  } bpp_;
  bool opt_bpp_log_ = false;                      // option "bpp_log": the log-space filter over the unfiltered plan
 public:
  std::vector<long long> last_prof;
 private:
};

Engine::Engine(const elemdp_model_desc& d)
    : au_(d.pattern ? d.pattern : ""), flags_(d.flags), max_span_(d.max_span), max_iloop_(d.max_iloop), min_bpp_(d.min_bpp),
      tau_(d.tau) {
  desc_ = d;
  desc_pattern_ = d.pattern ? d.pattern : "";
  desc_has_par_ = d.energy_param != nullptr;
  if (desc_has_par_) desc_par_ = d.energy_param;
  if ((flags_ & ELEMDP_NO_RSS) && (flags_ & ELEMDP_NO_PROFILE)) throw ArgError("no-rss, no-profile are exclusive.");
  if ((flags_ & ELEMDP_NO_RSS) && au_.reg_pattern().find(')') != std::string::npos)
    throw ArgError("search pattern must not include pair when no-rss mode");
  if (max_span_ < 1) throw ArgError("max_span must be positive");
  if (au_.S() > 128) throw ArgError("pattern has more than 128 interval states (not supported by this build)");
  if (!(tau_ > 0)) throw ArgError("tau must be positive");
  std::string par = d.energy_param ? d.energy_param : "~T2004~";
  if (par == "~T2004~") par = read_file(default_data_dir() + "/turner2004.elempar");
  else if (par == "~A2007~") par = read_file(default_data_dir() + "/andronescu2007.elempar");
  parse_energy_text(par, &et_);
  if (const char* e = getenv("ELEMDP_POISON")) opt_poison_ = e[0] == '1';   // (the test-suite sets it: see poison_tables)
  flatten_trivial(&lay0_, &ints0_);
  // the linear schedule needs state 0 = (0,0) to be closed under every transition family (decided before the automaton is
  // flattened: the shadow copy of (0,0) is only built for a closed state)
  linear_ok_ = au_.state(0).l == 0 && au_.state(0).r == 0;
  for (int c : au_.right(0)) linear_ok_ = linear_ok_ && c == 0;
  for (int c : au_.left(0)) linear_ok_ = linear_ok_ && c == 0;
  for (int c : au_.pair(0)) linear_ok_ = linear_ok_ && c == 0;
  for (auto const& sp : au_.splits(0)) linear_ok_ = linear_ok_ && sp[0] == 0 && sp[1] == 0;
  for (auto const& q : au_.quads()) if (q[0] == 0) linear_ok_ = linear_ok_ && q[1] == 0 && q[2] == 0 && q[3] == 0;
  flatten_automaton();

  int ndev = 0;
  has_device_ = hipGetDeviceCount(&ndev) == hipSuccess && ndev > 0;
  want_device_ = d.device;
  // Without a GPU the handle still serves the host-only calls (describe, initial_params,
  // train_finish); everything that computes raises ELEMDP_ENODEV -- there is no CPU path.
  if (has_device_) init_device();
}

// the flat transition lists of the pattern automaton (pruned to the transitions that can occur in a complete parse unless
// option "prune" = 0) and of its restriction to state (0,0)
void Engine::flatten_automaton() {
  au_.flatten(&lay_, &ints_, false, opt_prune_, false);
  au_.flatten(&layr_, &intsr_, true, opt_prune_, false);
  if (linear_ok_ && au_.S() < 127) au_.flatten(&lays_, &intss_, false, opt_prune_, true);
  else { lays_ = lay_; lays_.shadow = -1; intss_ = ints_; }
}

void Engine::upload_automaton() {
  d_ints_.upload(ints_, st_);
  d_intsr_.upload(intsr_, st_);
  d_lay_.alloc(sizeof(AutomatonLayout));
  d_layr_.alloc(sizeof(AutomatonLayout));
  d_lays_.alloc(sizeof(AutomatonLayout));
  d_intss_.upload(intss_, st_);
  HIP_OK(hipMemcpyAsync(d_lay_.as<void>(), &lay_, sizeof(AutomatonLayout), hipMemcpyHostToDevice, st_));
  HIP_OK(hipMemcpyAsync(d_layr_.as<void>(), &layr_, sizeof(AutomatonLayout), hipMemcpyHostToDevice, st_));
  HIP_OK(hipMemcpyAsync(d_lays_.as<void>(), &lays_, sizeof(AutomatonLayout), hipMemcpyHostToDevice, st_));
  HIP_OK(hipStreamSynchronize(st_));
}

void Engine::require_device() const {
  if (!has_device_) throw HipError("no HIP device available (libelemdp has no CPU path)");
}

void Engine::init_device() {
  if (want_device_ >= 0) { device_ = want_device_; HIP_OK(hipSetDevice(device_)); }
  else HIP_OK(hipGetDevice(&device_));
  hipDeviceProp_t prop;
  HIP_OK(hipGetDeviceProperties(&prop, device_));
  n_cu_ = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  HIP_OK(hipStreamCreateWithFlags(&st_, hipStreamNonBlocking));
  gs_[0] = st_;
  for (auto& e : gdone_) HIP_OK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  HIP_OK(hipEventCreateWithFlags(&gstart_, hipEventDisableTiming));
  for (auto& e : ev_) HIP_OK(hipEventCreate(&e));
  d_et_.alloc(sizeof(EnergyTables));
  HIP_OK(hipMemcpyAsync(d_et_.as<void>(), &et_, sizeof(EnergyTables), hipMemcpyHostToDevice, st_));
  loops_finite_ = loop_tables_finite(et_);
  {   // Boltzmann weights of the loop tables, for the BPP filter (energy_rules.h: loop_weight)
    std::unique_ptr<EnergyTables> x(new EnergyTables);
    exp_tables(et_, x.get());
    d_xet_.alloc(sizeof(EnergyTables));
    HIP_OK(hipMemcpy(d_xet_.as<void>(), x.get(), sizeof(EnergyTables), hipMemcpyHostToDevice));
    std::unique_ptr<BppCandTable> ct(new BppCandTable);
    build_bpp_cand(*x, ct.get());
    bpp_.cand.alloc(sizeof(BppCandTable));
    HIP_OK(hipMemcpy(bpp_.cand.as<void>(), ct.get(), sizeof(BppCandTable), hipMemcpyHostToDevice));
  }
  d_ints0_.upload(ints0_, st_);
  upload_automaton();
  d_lay0_.alloc(sizeof(AutomatonLayout));
  d_lin_.alloc(sizeof(double) * (kLinEth + au_.n_theta() + 1));
  HIP_OK(hipMemcpyAsync(d_lay0_.as<void>(), &lay0_, sizeof(AutomatonLayout), hipMemcpyHostToDevice, st_));
  d_params_.alloc(sizeof(ParamBlock) + sizeof(double) * (au_.n_theta() + 1));
  d_params0_.alloc(sizeof(ParamBlock) + sizeof(double));
  d_counter_.alloc(sizeof(int32_t));
  d_partial_.alloc(sizeof(double) * partial_len());
  {  // parameters of the one-state automaton of the BPP filter: lambda = 1, no emissions
    ParamBlock pb;
    pb.lambda[0] = pb.lambda[1] = 1.;
    pb.log_tau = 0.;
    pb.lam_same = 1;
    pb.pad = 0;
    HIP_OK(hipMemcpyAsync(d_params0_.as<void>(), &pb, sizeof(pb), hipMemcpyHostToDevice, st_));
  }
  HIP_OK(hipStreamSynchronize(st_));
}

void Engine::comm_init(int rank, int world, const void* id) {
  require_device();
  if (!id || world < 1 || rank < 0 || rank >= world) throw ArgError("elemdp_comm_init: bad rank / world / id");
  Rccl& r = Rccl::get();
  if (!r.ok()) throw HipError("no HIP device available for the collective: librccl.so could not be loaded");
  DeviceGuard dg(device_);
  comm_destroy();
  Rccl::UniqueId uid;
  std::memcpy(&uid, id, sizeof(uid));
  RCCL_OK(r.CommInitRank(&comm_, world, uid, rank));
  comm_rank_ = rank;
  comm_world_ = world;
}

void Engine::comm_destroy() {
  if (comm_) { DeviceGuard dg(device_); (void)Rccl::get().CommDestroy(comm_); comm_ = nullptr; comm_world_ = 1; comm_rank_ = 0; }
}

Engine::~Engine() {
  if (!has_device_) return;
  DeviceGuard dg(device_);
  comm_destroy();
  if (st_) (void)hipStreamSynchronize(st_);
  for (auto& e : ev_) if (e) (void)hipEventDestroy(e);
  for (int k = 0; k < kMaxGroupStreams; ++k) {
    if (gdone_[k]) (void)hipEventDestroy(gdone_[k]);
    if (k && gs_[k]) (void)hipStreamDestroy(gs_[k]);
  }
  if (gstart_) (void)hipEventDestroy(gstart_);
  if (st_) (void)hipStreamDestroy(st_);
}

void Engine::set_option(const std::string& key, double v) {
  if (key == "max_resident") { opt_max_resident_ = (int)v; return; }
  if (key == "slots") opt_slots_ = (int)v;
  else if (key == "keep_lnbpp") opt_keep_lnbpp_ = v != 0;
  else if (key == "first_pass_only") opt_first_pass_only_ = v != 0;
  else if (key == "profile") opt_profile_ = v != 0;
  else if (key == "two_streams") {}   // (retired with pipeline 2: accepted and ignored, as bench.py --serial-passes still sets it)
  else if (key == "group_streams") opt_group_streams_ = (int)v;
  else if (key == "pipeline") {
    if ((int)v != 3 && (int)v != 4) throw ArgError("option pipeline: 4 (scaled linear, default) or 3 (log space); the fused kernel (2) is retired");
    opt_pipeline_ = (int)v;
  }
  else if (key == "group") opt_group_ = (int)v;
  else if (key == "node_rules") {   // (node_profile: the emitting rules that take part, NodeRule bits; a subset gives that part of the profile)
    if (v < 1 || v > NR_ALL) throw ArgError("node_rules: 1 .. 63 (bits: L <- L, rule 3a, rule 5a, left base of rules 1a / 1b, rule 8, right base of rules 1a / 1b)");
    opt_node_rules_ = (int)v;
  }
  else if (key == "access_terms") {   // (accessibility: the terms that take part, bit AccessTerm; a subset gives that part of the sum)
    if (v < 1 || v > 15) throw ArgError("access_terms: 1 .. 15 (bits: loop runs, exterior, tails behind a branch, leading bases of a multi-loop)");
    opt_access_terms_ = (int)v;
  }
  else if (key == "schedule") opt_schedule_ = (int)v;
  else if (key == "dbg") opt_dbg_ = (int)v;
  else if (key == "bpp_log") opt_bpp_log_ = v != 0;
  else if (key == "poison") opt_poison_ = v != 0;
  else if (key == "world") {   // (the scan family's posterior products: the mixture, the parses with the motif, those without it)
    if (v != 0 && v != 1 && v != 2) throw ArgError("world: 0 (mixture, default), 1 (motif) or 2 (none)");
    opt_world_ = (int)v;
  }
  else if (key == "own_slots") opt_own_slots_ = v != 0;
  else if (key == "fast") opt_fast_ = v != 0;
  else if (key == "deterministic") opt_det_ = v != 0;
  else if (key == "sorted_plan") opt_sorted_plan_ = v != 0;
  else if (key == "useful_mask") opt_useful_mask_ = v != 0;
  else if (key == "pair_terms") opt_pair_terms_ = v != 0;
  else if (key == "live_blocks") {
    if (v < 0 || v > 2) throw ArgError("live_blocks: 0, 1 or 2");
    opt_live_blocks_ = (int)v;
  }
  else if (key == "loop_prepass") opt_loop_prepass_ = v != 0;
  else if (key == "loop_outside") opt_loop_outside_ = v != 0;
  else if (key == "live_span") {   // (0: the default; a model with more cells per block than the value takes its cells per block)
    if (v < 0 || v > lin_live_span_max()) throw ArgError("live_span: 0 (default) or cells per block .. " + std::to_string(lin_live_span_max()));
    opt_live_span_ = (int)v;
  }
  else if (key == "useful_mask_lds_kb") {   // (at most what a workgroup can have; takes effect for the masks built after it)
    if (v < 0 || v > 150) throw ArgError("useful_mask_lds_kb: 0 .. 150");
    opt_useful_lds_kb_ = (int)v;
  }
  else if (key == "eval_first") opt_eval_first_ = (int)v;
  else if (key == "eval_count") opt_eval_count_ = (int)v;
  else if (key == "prune") {
    opt_prune_ = v != 0;
    slots_.invalidate();   // (row widths and the pair list follow the transition lists)
    flatten_automaton();
    if (has_device_) { DeviceGuard dg(device_); HIP_OK(hipStreamSynchronize(st_)); upload_automaton(); }
  }
  else throw ArgError("unknown option: " + key);
  if (key != "world") for (auto& m : st_mask_) m.clear();   // (an option may change the filter: cached masks of a streamed batch go)
  // (replayed on the inner engines of a streamed batch; world, set around every call, takes one entry however often it is set)
  auto at = key == "world" ? std::find_if(opt_log_.begin(), opt_log_.end(), [&](const std::pair<std::string, double>& kv) { return kv.first == key; })
                           : opt_log_.end();
  if (at != opt_log_.end()) at->second = v;
  else opt_log_.emplace_back(key, v);
  for (auto& e : sub_) if (e) e->set_option(key, v);
}

void Engine::set_theta_from(const double* x) {
  const int nt = au_.n_theta();
  theta_.assign(x, x + nt);
  if (softmax()) {  // theta = log-softmax of the score rows (ProfileHMM::calc_theta, profile_hmm.hpp:103-111)
    for (int r = 0; r < au_.n_rows(); ++r) {
      const int o = au_.row_offset(r), w = au_.row_width(r);
      double tot = -std::numeric_limits<double>::infinity();
      for (int c = 0; c < w; ++c) {  // logsumexp by sequential log1p(exp()) like util.hpp:195-209
        const double a = tot, b = x[o + c];
        tot = (b == -INFINITY) ? a : (a == -INFINITY) ? b : (a < b ? b + std::log1p(std::exp(a - b)) : a + std::log1p(std::exp(b - a)));
      }
      for (int c = 0; c < w; ++c) theta_[o + c] = x[o + c] - tot;
    }
  }
}

void Engine::upload_params(const double* x, const AutomatonLayout& lay, bool) {
  const int nt = au_.n_theta();
  set_theta_from(x);
  std::vector<double> blob(sizeof(ParamBlock) / sizeof(double) + nt + 1, 0.);
  ParamBlock pb;
  pb.lambda[0] = x[nt];
  pb.lambda[1] = x[nt + 1];
  pb.log_tau = std::log(tau_);
  pb.lam_same = (x[nt] == x[nt + 1]) ? 1 : 0;
  pb.pad = 0;
  std::memcpy(blob.data(), &pb, sizeof(pb));
  std::copy(theta_.begin(), theta_.end(), blob.begin() + sizeof(ParamBlock) / sizeof(double));
  HIP_OK(hipMemcpyAsync(d_params_.as<void>(), blob.data(), blob.size() * sizeof(double), hipMemcpyHostToDevice, st_));
  // linear parameter block (+ the weight tables of the table-driven unary phases) for the plain automaton and for the one
  // with the shadow state (their transition ids differ)
  make_lin_params(lay_, ints_.data(), theta_.data(), tau_, (flags_ & ELEMDP_NO_PROFILE) != 0, &h_lin_);
  d_lin_.alloc(sizeof(double) * (h_lin_.size() + 1));
  HIP_OK(hipMemcpyAsync(d_lin_.as<void>(), h_lin_.data(), h_lin_.size() * sizeof(double), hipMemcpyHostToDevice, st_));
  make_lin_params(lays_, intss_.data(), theta_.data(), tau_, (flags_ & ELEMDP_NO_PROFILE) != 0, &h_lins_);
  d_lins_.alloc(sizeof(double) * (h_lins_.size() + 1));
  HIP_OK(hipMemcpyAsync(d_lins_.as<void>(), h_lins_.data(), h_lins_.size() * sizeof(double), hipMemcpyHostToDevice, st_));
  HIP_OK(hipStreamSynchronize(st_));  // blob is a local
  (void)lay;
}

LdsLayout Engine::lds_layout(const AutomatonLayout& lay, int Lmax, int nword_max, bool scan) const {
  LdsLayout l;
  int o = 0;
  auto take = [&](int bytes) { int p = o; o += (bytes + 15) & ~15; return p; };
  l.theta = take(8 * (lay.n_theta + 1));
  l.en_o = take(8 * (lay.n_theta + 1));
  l.en_x = take(8 * (lay.n_theta + 1));
  l.eh = take(8 * 4);
  l.zs = take(8 * 8);
  l.ws = take(8 * (Lmax + 1));
  l.post = take(scan ? 8 * 3 * (Lmax + 1) : 16);
  l.ints = take(4 * lay.n_small);
  l.wave_scr = take(8 * 128 * (kThreads / 64));
  l.okbits = take(4 * nword_max);
  l.dmin = take(2 * (Lmax + 1));
  l.seq = take(Lmax + 1);
  l.unp = take(Lmax + 1);
  l.total = o;
  if (l.total > 160 * 1024) throw ArgError("sequence / pattern too large for the LDS staging of this build");
  return l;
}

// wall-clock laps on stderr when ELEMDP_TIME is set (where does a first call spend its time?)
static void dbg_lap(const char* what) {
  static const bool on = getenv("ELEMDP_TIME") != nullptr;
  static auto t0 = std::chrono::steady_clock::now();
  if (!on) return;
  const auto t1 = std::chrono::steady_clock::now();
  fprintf(stderr, "[elemdp %8.1f ms] %s\n", std::chrono::duration<double, std::milli>(t1 - t0).count(), what);
  t0 = t1;
}

void Engine::build_planset(PlanSet& ps, int first, int count, const uint32_t* d_okbits) {
  ps.first = first;
  ps.count = count;
  ps.h.assign(h_plans_.begin() + first, h_plans_.begin() + first + count);
  int64_t dmin_b = 0, cell_b = 0, off_b = 0, bits_end = 0, ncell_max = 0, blk_b = 0;
  int lmax = 0, wmax1 = 0;
  for (auto& p : ps.h) {
    const int64_t nc = (int64_t)(p.L + 1) * (p.W + 1);
    p.dmin_base = dmin_b; p.cell_base = cell_b; p.off_base = off_b; p.item_base = 0; p.n_items = 0;
    // (the lists are addressed by an int: a set too large for that gets none)
    p.blk_base = blk_b >= 0 ? (int32_t)blk_b : 0;
    if (blk_b >= 0) { blk_b += live_blocks_records(p.L, p.W); if (blk_b > 0x7fffffffll) blk_b = -1; }
    dmin_b += p.L + 1; cell_b += nc; off_b += nc + 1;
    bits_end = std::max<int64_t>(bits_end, p.bits_base + (nc + 31) / 32);
    ncell_max = std::max(ncell_max, nc);
    lmax = std::max(lmax, (int)p.L);
    wmax1 = std::max(wmax1, (int)p.W + 1);
  }
  ps.n_cells = cell_b;
  ps.n_blocks = blk_b;
  ps.useful_built = ps.pair_terms_built = false;   // (the mask follows the pair mask: ensure_useful_mask builds it again, and the pair terms behind it)
  ps.blk_cpb = ps.blk_cap = 0;   // (and the lists follow the mask)
  d_okbits_end_.alloc(sizeof(uint32_t) * (size_t)bits_end);   // the pair mask by (end, span): scratch of the item enumeration
  ps.d_plans.upload(ps.h, st_);
  const bool chunked = ps.inner_only;   // the plan of the unfiltered mask is rebuilt chunk after chunk: its buffers only grow
  ps.dmin.alloc(sizeof(int16_t) * dmin_b, chunked);
  for (DevBuf* b : {&ps.e_stack, &ps.e_ext, &ps.e_ml, &ps.e_close, &ps.e_hp}) b->alloc(sizeof(double) * cell_b, chunked);
  for (DevBuf* b : {&ps.off_outer, &ps.off_inner, &ps.off_left, &ps.off_right, &ps.cursor}) b->alloc(sizeof(int32_t) * off_b, chunked);
  d_nitems_.alloc(sizeof(int32_t) * count);
  PlanKernelArgs a;
  a.et = d_et_.as<EnergyTables>();
  a.b.seq = d_seq_.as<uint8_t>(); a.b.ws = d_ws_.as<double>(); a.b.unp = d_unp_.as<uint8_t>();
  a.b.ndot = ((flags_ & ELEMDP_DBG_FIX_RSS) || constrained_) ? d_ndot_.as<int32_t>() : nullptr;
  a.okbits = d_okbits;
  a.okbits_end = d_okbits_end_.as<uint32_t>();
  a.ncell_max = (int32_t)ncell_max;
  a.n_roles = ps.inner_only ? 1 : 3;
  a.lmax = lmax;
  a.wmax1 = wmax1;
  a.nword_max = (int32_t)((ncell_max + 31) / 32);
  a.plans = ps.d_plans.as<SeqPlan>();
  a.first = 0; a.count = count;
  a.p = ps.arrays();
  a.no_ene = (flags_ & ELEMDP_NO_ENERGY) ? 1 : 0;
  a.min_span = min_span();
  a.fix_rss = ((flags_ & ELEMDP_DBG_FIX_RSS) || constrained_) ? 1 : 0;   // (the plan builder reads ndot)
  a.count_fast = (loops_finite_ && !a.fix_rss && !getenv("ELEMDP_PLAN_ENUM_COUNT")) ? 1 : 0;
  HIP_OK(launch_plan_cells(a, d_nitems_.as<int32_t>(), st_));
  std::vector<int32_t> n_items(count);
  HIP_OK(hipMemcpyAsync(n_items.data(), d_nitems_.as<void>(), sizeof(int32_t) * count, hipMemcpyDeviceToHost, st_));
  HIP_OK(hipStreamSynchronize(st_));
  int64_t ib = 0;
  for (int k = 0; k < count; ++k) {
    ps.h[k].n_items = n_items[k]; ps.h[k].item_base = ib; ib += n_items[k];
    a.nitems_max = std::max(a.nitems_max, n_items[k]);
  }
  ps.n_items = ib;
  if (getenv("ELEMDP_PLAN_DEBUG")) fprintf(stderr, "planset: %d sequences, %lld items, largest %d, cells %lld\n", count, (long long)ib, a.nitems_max, (long long)ncell_max);
  ps.d_plans.upload(ps.h, st_);
  ps.items.alloc(sizeof(LoopItem) * ib, true);
  ps.item_in.alloc(ib, true);
  for (DevBuf* b : {&ps.idx_inner, &ps.idx_left, &ps.idx_right}) b->alloc(sizeof(int32_t) * ib, true);
  if (ps.permuted) for (DevBuf* b : {&ps.items_inner, &ps.items_left, &ps.items_right}) b->alloc(sizeof(LoopItem) * (ib + 1), true);
  a.plans = ps.d_plans.as<SeqPlan>();
  a.p = ps.arrays();
  // The scaled-linear pipeline adds over the role lists with atomics: their order inside a segment is immaterial, and the sort
  // is a quarter of the plan builder.  The log-space pipeline and the deterministic mode get it (here, or later through
  // ensure_sorted_plan when the option arrives after the batch).
  a.sort_roles = (ps.inner_only || opt_det_ || opt_pipeline_ != 4 || opt_sorted_plan_) ? 1 : 0;
  HIP_OK(launch_plan_items(a, st_));
  if (ps.permuted && !plan_copies_fused(a)) HIP_OK(launch_permute_items(a, st_));
  HIP_OK(hipStreamSynchronize(st_));
  ps.sorted = a.sort_roles != 0;
  ps.ka = a;
}

// The usefulness mask of the resident plan, from its pair masks and dmin (still in place: the band kernels read them too).
void Engine::ensure_useful_mask() {
  if (plan_.useful_built || plan_.count <= 0) return;
  plan_.useful.alloc((size_t)plan_.n_cells);
  plan_.ka.p.useful = plan_.useful.as<uint8_t>();
  plan_.ka.m_min = m_min();
  HIP_OK(launch_useful_mask(plan_.ka, (size_t)plan_.n_cells, (size_t)opt_useful_lds_kb_ * 1024, st_));
  plan_.useful_built = true;
  // the pair terms of the outside sweep: plan work like the mask they are read from (not from the mask of all ones, which drops
  // nothing, nor for a span that does not fit a word)
  plan_.pair_terms_built = false;
  plan_.ka.p.ha_rows = plan_.ka.p.h1_stems = nullptr;
  if (plan_.ka.wmax1 - 1 <= kPairTermsMaxW && useful_mask_fits(plan_.ka, (size_t)opt_useful_lds_kb_ * 1024)) {
    plan_.pair_words.alloc(2 * sizeof(unsigned long long) * (size_t)plan_.n_cells);
    plan_.ka.p.ha_rows = plan_.pair_words.as<unsigned long long>();
    plan_.ka.p.h1_stems = plan_.ka.p.ha_rows + (size_t)plan_.n_cells;
    HIP_OK(launch_pair_terms(plan_.ka, st_));
    plan_.pair_terms_built = true;
  }
  plan_.blk_cpb = plan_.blk_cap = 0;
  ++plan_gen_;
}

// The live-block lists of the resident plan for blocks of `cpb` cells that span at most `cap`, from its mask; the largest block
// count per diagonal is read back once (W + 1 ints: the grids of the train sweeps).  False: no lists for this plan / geometry.
// inside_too: also the second set, for the inside sweep behind the loop pre-pass (without it one set, as before the pre-pass).
bool Engine::ensure_live_blocks(int cpb, int cap, bool inside_too) {
  if (plan_.count <= 0 || plan_.n_blocks <= 0 || cpb < kLiveCpbMin || cap < cpb || cap > kLiveSpanMax) return false;
  ensure_useful_mask();
  if (plan_.blk_cpb == cpb && plan_.blk_cap == cap && plan_.blk_all == (opt_live_blocks_ >= 2) && (plan_.blk_two || !inside_too)) return true;
  plan_.blocks.alloc(sizeof(LiveBlock) * (inside_too ? 2 : 1) * (size_t)plan_.n_blocks);   // (one set or both: live_blocks.h)
  plan_.blk_max.alloc(sizeof(int32_t) * 6 * (size_t)plan_.ka.wmax1);
  PlanKernelArgs a = plan_.ka;
  a.p.useful = plan_.useful.as<uint8_t>();
  a.p.blocks = plan_.blocks.as<LiveBlock>();
  a.p.blocks_in = inside_too ? a.p.blocks + (size_t)plan_.n_blocks : nullptr;
  a.blk_max = plan_.blk_max.as<int32_t>();
  a.live_cpb = cpb; a.live_cap = cap;
  HIP_OK(launch_live_blocks(a, (size_t)plan_.n_blocks, st_));
  plan_.h_blk_max.assign(6 * (size_t)a.wmax1, 0);
  HIP_OK(hipMemcpyAsync(plan_.h_blk_max.data(), a.blk_max, sizeof(int32_t) * 6 * (size_t)a.wmax1, hipMemcpyDeviceToHost, st_));
  HIP_OK(hipStreamSynchronize(st_));
  // the grid of every diagonal: its largest block count, or -1 where the lists leave too many of the workgroups (kLiveKeepPct)
  // (each direction its own: the inside sweep behind the loop pre-pass takes the second set)
  plan_.h_blk_grid.assign((size_t)a.wmax1, 0);
  plan_.h_blk_grid_in.assign((size_t)a.wmax1, 0);
  for (int d = 0; d < a.wmax1; ++d) {
    const int32_t* mi = plan_.h_blk_max.data() + 3 * (size_t)a.wmax1;
    const long long nb = plan_.h_blk_max[a.wmax1 + d], nw = plan_.h_blk_max[2 * a.wmax1 + d];
    const long long nbi = mi[a.wmax1 + d], nwi = mi[2 * a.wmax1 + d];
    plan_.h_blk_grid[d] = (opt_live_blocks_ >= 2 || nb * 100 <= nw * kLiveKeepPct) ? plan_.h_blk_max[d] : -1;
    plan_.h_blk_grid_in[d] = (opt_live_blocks_ >= 2 || nbi * 100 <= nwi * kLiveKeepPct) ? mi[d] : -1;
    if (getenv("ELEMDP_PLAN_DEBUG"))
      fprintf(stderr, "live blocks d %d: most %d, blocks %lld, working without lists %lld%s; inside behind the loop pre-pass: most %d, blocks %lld, working without lists %lld%s\n",
              d, plan_.h_blk_max[d], nb, nw, plan_.h_blk_grid[d] < 0 ? " (consecutive)" : "", mi[d], nbi, nwi, plan_.h_blk_grid_in[d] < 0 ? " (consecutive)" : "");
  }
  plan_.blk_all = opt_live_blocks_ >= 2;
  plan_.blk_two = inside_too;
  plan_.blk_cpb = cpb; plan_.blk_cap = cap;
  ++plan_gen_;
  return true;
}

void Engine::ensure_sorted_plan() {
  if (plan_.sorted || plan_.count <= 0) return;
  HIP_OK(launch_plan_sort(plan_.ka, st_));
  if (plan_.permuted) HIP_OK(launch_permute_items(plan_.ka, st_));
  HIP_OK(hipStreamSynchronize(st_));
  plan_.sorted = true;
  ++plan_gen_;
}

SlotRequest Engine::slot_request(int S, int row, bool scan, int n_want, int group, int pair_row) const {
  SlotRequest r;
  r.S = S; r.row = row; r.scan = scan; r.n_want = n_want; r.group = group; r.pair_row = pair_row;
  r.opt_slots = opt_slots_; r.n_cu = n_cu_;
  r.Lmax = Lmax_; r.Wmax = Wmax_; r.S_dense = au_.S();
  r.budget = slot_budget_;
  return r;
}

DpArgs Engine::base_args(const AutomatonLayout& lay, const int32_t* d_ints, const double* d_params, const PlanSet& ps,
                         const uint32_t* d_okbits, int S) {
  DpArgs a;
  std::memset(&a, 0, sizeof(a));
  a.lay = lay;
  a.layp = (&lay == &lay0_) ? d_lay0_.as<AutomatonLayout>() : d_lay_.as<AutomatonLayout>();
  a.ints = d_ints;
  a.params = d_params;
  a.no_prf = (flags_ & ELEMDP_NO_PROFILE) ? 1 : 0;
  a.m_min = m_min();
  a.no_rss = (flags_ & ELEMDP_NO_RSS) ? 1 : 0;
  a.plans = ps.d_plans.as<SeqPlan>();
  a.n_seq = ps.count;
  a.counter = d_counter_.as<int32_t>();
  a.b.seq = d_seq_.as<uint8_t>(); a.b.ws = d_ws_.as<double>(); a.b.unp = d_unp_.as<uint8_t>();
  a.b.ndot = nullptr;
  a.okbits = d_okbits;
  a.p = ps.arrays();
  a.band_in = slots_.band_in.as<double>(); a.band_out = slots_.band_out.as<double>();
  a.ext_in = slots_.ext_in.as<double>(); a.ext_out = slots_.ext_out.as<double>();
  a.band_stride = (size_t)kNumBandStates * (Wmax_ + 1) * (Lmax_ + 1) * S;
  a.ext_stride = (size_t)(Lmax_ + 1) * S;
  a.tmp = slots_.tmp.as<double>();
  a.tmp_stride = a.ext_stride;
  return a;
}

// load_batch: check; stream, or stage and upload; canonical mask; BPP filter; resident plan; commit.  A rejected batch leaves the
// handle without a batch (ELEMDP_ESTATE for what follows) instead of the new sizes over the old device buffers.
void Engine::load_batch(const uint8_t* seq, const int32_t* off, const uint8_t* qual, const int32_t* qoff, const char* fix,
                        int n, const char* cons) {
  require_device();
  DeviceGuard dg(device_);
  n_seq_ = 0;
  pairs_.invalidate();
  conds_.invalidate();
  stems_.invalidate();
  helices_.invalidate();
  loops_.invalidate();
  streaming_ = false;
  train_rows_ = false;
  constrained_ = false;   // (until the filter is through: it and the plan of its unfiltered mask see no constraint)
  if (cons && (flags_ & (ELEMDP_DBG_FIX_RSS | ELEMDP_NO_RSS)))
    throw ArgError("load_batch: constraints go with neither ELEMDP_DBG_FIX_RSS nor ELEMDP_NO_RSS");
  BatchShape shape = check_batch(seq, off, qual, qoff, fix, n);
  // strings that constrain nothing (every character '.'): a plain load, with its popcount count pass and no extra buffer
  if (cons && std::all_of(cons + off[0], cons + off[n], [](char c) { return c == '.'; })) cons = nullptr;
  if (!cons) { d_cons_cls_.reset(); d_cons_partner_.reset(); d_cons_enc_.reset(); d_okbits_f_.reset(); }
  ConsRows rows;
  // (a streamed batch derives the rows chunk by chunk on its inner handles: the outer handle only checks the strings, so that a
  // refusal comes at the load and names the sequence by its index in the whole batch)
  const bool stream = should_stream(shape);
  if (cons) rows = constraint_rows(shape, seq, off, cons, stream);
  h_seq_off_.assign(off, off + n + 1);
  h_qual_off_.assign(qoff, qoff + n + 1);
  if (cons) st_cons_.assign(cons + off[0], cons + off[n]); else st_cons_.clear();
  if (stream) { stream_setup(seq, off, qual, qoff, fix, std::move(shape)); return; }
  st_cons_.clear();
  std::vector<uint8_t> h_seq;      // (becomes h_seq_ at the commit)
  std::vector<uint32_t> fix_bits;  // (ELEMDP_DBG_FIX_RSS: the pairs of the fixed structures)
  stage_batch(std::move(shape), seq, off, qual, qoff, fix, h_seq, fix_bits);
  // ---- canonical mask (d_okbits0_); it also counts the possible pairs = the denominator of bpp_eff
  const bool rss = !(flags_ & ELEMDP_DBG_FIX_RSS) && !(flags_ & ELEMDP_NO_RSS);
  d_ncanon_.alloc(sizeof(int32_t) * n);
  d_plans_all_.upload(h_plans_, st_);
  BatchArrays b;
  b.seq = d_seq_.as<uint8_t>(); b.ws = d_ws_.as<double>(); b.unp = d_unp_.as<uint8_t>(); b.ndot = nullptr;
  HIP_OK(launch_mask(b, d_plans_all_.as<SeqPlan>(), n, min_span(), rss, d_okbits0_.as<uint32_t>(), d_ncanon_.as<int32_t>(), st_));
  std::vector<int32_t> ncanon(n);
  HIP_OK(hipMemcpyAsync(ncanon.data(), d_ncanon_.as<void>(), sizeof(int32_t) * n, hipMemcpyDeviceToHost, st_));
  HIP_OK(hipStreamSynchronize(st_));
  for (int k = 0; k < n; ++k) h_plans_[k].n_canonical = ncanon[k];
  dbg_lap("load: uploads + canonical mask");
  const uint32_t* mask = bpp_filter(fix_bits);
  resident_plan(cons ? constrain(mask, rows) : mask);
  h_seq_.swap(h_seq);
  n_seq_ = n;   // committed: everything above succeeded
  opt_eval_first_ = opt_eval_count_ = 0;   // (an evaluation range belongs to the batch it was set for)
  range_key_[0] = range_key_[1] = -1;
}

// the one check of a batch, resident or streamed (writes no member)
Engine::BatchShape Engine::check_batch(const uint8_t* seq, const int32_t* off, const uint8_t* qual, const int32_t* qoff,
                                       const char* fix, int n) const {
  if (n <= 0 || !seq || !off || !qual || !qoff) throw ArgError("load_batch: empty batch or null pointer");
  if ((flags_ & ELEMDP_DBG_FIX_RSS) && !fix) throw ArgError("load_batch: ELEMDP_DBG_FIX_RSS needs fix_rss strings");
  BatchShape b;
  b.plans.assign(n, SeqPlan());
  for (int k = 0; k < n; ++k) {
    const int L = off[k + 1] - off[k];
    if (L <= 0) throw ArgError("load_batch: empty sequence");
    if (L > 32000) throw ArgError("load_batch: sequence longer than 32000");
    if (qoff[k + 1] - qoff[k] != L + 1) throw ArgError("bad seq format. (quality must have L+1 entries)");  // motif_trainer.hpp:139
    uint8_t cmax = 0;   // (a max, not a search: it vectorises)
    for (int t = 0; t < L; ++t) cmax = std::max(cmax, seq[off[k] + t]);
    if (cmax > 4) throw ArgError("load_batch: base code out of range");
    SeqPlan& p = b.plans[k];
    p.L = L;
    p.W = std::min(L, max_span_);
    p.C = std::min(p.W - 2 - ((flags_ & ELEMDP_DBG_NO_TURN) ? 2 : 5), max_iloop_);  // energy_model.hpp:271-273
    p.positive = qual[qoff[k + 1] - 1] == 0;
    p.seq_base = b.n_bases; p.pos_base = b.n_pos; p.bits_base = b.n_words;
    const int64_t nc = (int64_t)(L + 1) * (p.W + 1);
    const int nword = (int)((nc + 31) / 32);
    b.n_bases += L; b.n_pos += L + 1; b.n_words += nword; b.n_cells += nc;
    b.Lmax = std::max(b.Lmax, L); b.Wmax = std::max(b.Wmax, p.W); b.nword_max = std::max(b.nword_max, nword);
  }
  if ((double)kNumBandStates * (b.Wmax + 1) * (b.Lmax + 1) * au_.S() >= 2147483648.0)
    throw ArgError("load_batch: sequence too long for this pattern (band table exceeds 2^31 entries)");
  return b;
}

// the rows of the constraint strings (concatenated, indexed as the sequences); throws on a string §26 refuses.  check_only: the
// strings are checked and no rows are kept (every sequence writes the same scratch of the longest one)
Engine::ConsRows Engine::constraint_rows(const BatchShape& b, const uint8_t* seq, const int32_t* off, const char* cons,
                                         bool check_only) const {
  ConsRows r;
  const size_t pos_b = check_only ? (size_t)b.Lmax + 1 : (size_t)b.n_pos;
  r.cls.assign(pos_b, 0); r.unp.assign(pos_b, 1); r.partner.assign(pos_b, -1); r.enc.assign(pos_b, -1); r.ndot.assign(pos_b, 0);
  for (size_t k = 0; k < b.plans.size(); ++k) {
    const SeqPlan& p = b.plans[k];
    const uint8_t* s = seq + off[k];
    const size_t at = check_only ? 0 : (size_t)p.pos_base;
    const auto pair_ok = [&](int i, int j) { return canonical_pair(s, p.L, p.W, min_span(), i, j - i + 1); };
    const std::string err = constraint_derive(cons + off[k], p.L, (int)k, pair_ok, &r.cls[at], &r.partner[at], &r.enc[at], &r.unp[at],
                                              &r.ndot[at]);
    if (!err.empty()) throw ArgError(err);
  }
  if (check_only) r = ConsRows();
  return r;
}

// Behind the BPP filter: the constrained mask in d_okbits1_ (k_constrain, from the filter's mask wherever it lies), and the unp /
// ndot rows of the constraint in place of the all-ones row the filter read.  The inner handle of a streamed batch keeps the
// filter's own mask in d_okbits_f_ for the cache (filter_result); a resident batch needs no copy of it.
const uint32_t* Engine::constrain(const uint32_t* mask, const ConsRows& rows) {
  if (inner_ && mask == d_okbits1_.as<uint32_t>()) {
    d_okbits_f_.alloc(sizeof(uint32_t) * bits_words_);
    HIP_OK(hipMemcpyAsync(d_okbits_f_.as<void>(), mask, sizeof(uint32_t) * bits_words_, hipMemcpyDeviceToDevice, st_));
    mask = d_okbits_f_.as<uint32_t>();
  }
  d_cons_cls_.upload(rows.cls, st_); d_cons_partner_.upload(rows.partner, st_); d_cons_enc_.upload(rows.enc, st_);
  d_unp_.upload(rows.unp, st_); d_ndot_.upload(rows.ndot, st_);
  HIP_OK(launch_constrain(d_plans_all_.as<SeqPlan>(), (int)h_plans_.size(), nword_max_, d_cons_cls_.as<uint8_t>(),
                          d_cons_partner_.as<int32_t>(), d_cons_enc_.as<int32_t>(), mask, d_okbits1_.as<uint32_t>(), st_));
  HIP_OK(hipStreamSynchronize(st_));   // (the rows are host vectors of the caller's)
  constrained_ = true;
  dbg_lap("load: constraint mask");
  return d_okbits1_.as<uint32_t>();
}

// the batch arrays on the host (base codes into h_seq, the rest through the pinned staging) and their uploads on st_
void Engine::stage_batch(BatchShape&& b, const uint8_t* seq, const int32_t* off, const uint8_t* qual, const int32_t* qoff,
                         const char* fix, std::vector<uint8_t>& h_seq, std::vector<uint32_t>& fix_bits) {
  const int n = (int)b.plans.size();
  const bool fixmode = flags_ & ELEMDP_DBG_FIX_RSS;
  h_plans_ = std::move(b.plans);
  Lmax_ = b.Lmax; Wmax_ = b.Wmax; nword_max_ = b.nword_max;
  bits_words_ = (size_t)b.n_words;
  n_cells_total_ = b.n_cells;
  const size_t pos_b = (size_t)b.n_pos;
  h_seq.resize((size_t)b.n_bases);
  uint8_t* h_unp = hb_unp_.get<uint8_t>(pos_b);
  double* h_ws = hb_ws_.get<double>(pos_b);
  double* h_ews = hb_ews_.get<double>(pos_b);
  std::memset(h_unp, 1, pos_b);
  std::vector<int32_t> h_ndot;
  if (fixmode) { h_ndot.assign(pos_b, 0); fix_bits.assign(bits_words_, 0u); }
  for (int k = 0; k < n; ++k) {
    const SeqPlan& p = h_plans_[k];
    std::memcpy(&h_seq[p.seq_base], seq + off[k], p.L);
    position_weights(qual + qoff[k], p.L + 1, &h_ws[p.pos_base], &h_ews[p.pos_base]);
    if (!fixmode) continue;
    const char* f = fix + off[k];
    nondot_prefix(f, p.L, &h_ndot[p.pos_base]);
    std::vector<int> open;
    for (int t = 0; t < p.L; ++t) {
      h_unp[p.pos_base + t] = f[t] == '.';
      if (f[t] == '(') open.push_back(t);
      else if (f[t] == ')') {
        if (open.empty()) throw ArgError("bad rss: unbalanced");
        const int o = open.back();
        open.pop_back();
        const int d = t + 1 - o;
        if (d > p.W) throw ArgError("bad rss: pair wider than max_span");
        const int64_t c = (int64_t)o * (p.W + 1) + d;
        fix_bits[p.bits_base + (c >> 5)] |= 1u << (c & 31);
      } else if (f[t] != '.') throw ArgError(std::string("bad rss char: ") + f[t]);
    }
    if (!open.empty()) throw ArgError("bad rss: unbalanced");
  }
  dbg_lap("load: host arrays");
  h_order_.resize(n);
  std::iota(h_order_.begin(), h_order_.end(), 0);
  std::stable_sort(h_order_.begin(), h_order_.end(), [&](int a, int c) { return h_plans_[a].L > h_plans_[c].L; });
  d_seq_.upload(h_seq, st_);
  d_ws_.alloc(sizeof(double) * pos_b);
  HIP_OK(hipMemcpyAsync(d_ws_.as<void>(), h_ws, sizeof(double) * pos_b, hipMemcpyHostToDevice, st_));
  d_ews_.alloc(sizeof(double) * pos_b);
  HIP_OK(hipMemcpyAsync(d_ews_.as<void>(), h_ews, sizeof(double) * pos_b, hipMemcpyHostToDevice, st_));
  d_unp_.alloc(pos_b);
  HIP_OK(hipMemcpyAsync(d_unp_.as<void>(), h_unp, pos_b, hipMemcpyHostToDevice, st_));
  if (fixmode) d_ndot_.upload(h_ndot, st_);
  d_okbits0_.alloc(sizeof(uint32_t) * bits_words_);
  d_okbits1_.alloc(sizeof(uint32_t) * bits_words_);
}

// The BPP filter (energy_model.hpp:249-265): bpp_eff of every sequence, and the pair mask the resident plan is built over --
// d_okbits1_ where the filter ran (or a streamed batch's cache stood in for it), else the canonical / fixed / empty d_okbits0_.
const uint32_t* Engine::bpp_filter(const std::vector<uint32_t>& fix_bits) {
  const bool no_rss = flags_ & ELEMDP_NO_RSS, fixmode = flags_ & ELEMDP_DBG_FIX_RSS;
  const uint32_t* preset_bits = preset_words_ == bits_words_ ? preset_bits_ : nullptr;
  const double* preset_eff = preset_eff_;
  preset_bits_ = nullptr; preset_eff_ = nullptr; preset_words_ = 0;
  h_lnbpp_.clear(); h_lnbpp_base_.clear();
  // the filter's result from an earlier load of the same records (streamed batch)
  if (preset_bits && !no_rss && !fixmode && min_bpp_ > 0 && !opt_keep_lnbpp_) {
    HIP_OK(hipMemcpyAsync(d_okbits1_.as<void>(), preset_bits, sizeof(uint32_t) * bits_words_, hipMemcpyHostToDevice, st_));
    HIP_OK(hipStreamSynchronize(st_));
    for (size_t k = 0; k < h_plans_.size(); ++k) h_plans_[k].bpp_eff = preset_eff[k];
    dbg_lap("load: filtered mask from the cache");
    return d_okbits1_.as<uint32_t>();
  }
  if (no_rss) {
    HIP_OK(hipMemsetAsync(d_okbits0_.as<void>(), 0, sizeof(uint32_t) * bits_words_, st_));
    for (auto& p : h_plans_) p.bpp_eff = 0.;  // em.set_seq is never called in --no-rss mode (motif_model.hpp:57)
  } else if (fixmode) {
    HIP_OK(hipMemcpyAsync(d_okbits0_.as<void>(), fix_bits.data(), sizeof(uint32_t) * bits_words_, hipMemcpyHostToDevice, st_));
    HIP_OK(hipStreamSynchronize(st_));
    for (auto& p : h_plans_) {
      int nbp = 0;
      const int nword = (int)(((int64_t)(p.L + 1) * (p.W + 1) + 31) / 32);
      for (int w = 0; w < nword; ++w) nbp += __builtin_popcount(fix_bits[p.bits_base + w]);
      p.bpp_eff = (double)nbp / (double)p.n_canonical;
    }
  } else if (min_bpp_ > 0) {
    bpp_chunks(Wmax_ <= kBppLinMaxSpan && !opt_bpp_log_);   // the linear form, or log space (bands too wide; option "bpp_log")
    return d_okbits1_.as<uint32_t>();
  } else {
    for (auto& p : h_plans_) p.bpp_eff = 1.;  // 0 == min_BPP: nbp = total (energy_model.hpp:249-251)
  }
  return d_okbits0_.as<uint32_t>();
}

// K1 chunk after chunk: the form writes the kept pairs to d_okbits1_, their count to bpp_.kept, ln BPP per cell to lnbpp
void Engine::bpp_chunks(bool lin) {
  const int n = (int)h_plans_.size();
  // cells per chunk, bounded by the filter's memory: the linear form holds 23 doubles per cell (~12 GB per chunk), the log-space
  // form a plan of the unfiltered mask (a few GB)
  const int64_t cells_cap = (lin ? 64LL : 24LL) * 1000 * 1000;
  if (opt_keep_lnbpp_) h_lnbpp_base_.assign(n + 1, 0);
  for (int first = 0, count = 0; first < n; first += count) {
    int64_t cells = 0;
    for (count = 0; first + count < n; ++count) {
      const int64_t nc = (int64_t)(h_plans_[first + count].L + 1) * (h_plans_[first + count].W + 1);
      if (count > 0 && cells + nc > cells_cap) break;
      cells += nc;
    }
    bpp_.kept.alloc(sizeof(int32_t) * count, true);
    DevBuf d_lnbpp;
    if (opt_keep_lnbpp_) d_lnbpp.alloc(sizeof(double) * cells);
    if (lin) bpp_lin_chunk(first, count, cells, d_lnbpp.as<double>());
    else bpp_log_chunk(first, count, cells, d_lnbpp.as<double>());
    std::vector<int32_t> kept(count);
    HIP_OK(hipMemcpyAsync(kept.data(), bpp_.kept.as<void>(), sizeof(int32_t) * count, hipMemcpyDeviceToHost, st_));
    HIP_OK(hipStreamSynchronize(st_));
    for (int k = 0; k < count; ++k) h_plans_[first + k].bpp_eff = (double)kept[k] / (double)h_plans_[first + k].n_canonical;
    dbg_lap(lin ? "load: BPP filter, linear (chunk)" : "load: BPP filter (chunk)");
    if (opt_keep_lnbpp_) {   // (cells of a chunk in sequence order)
      const size_t base = h_lnbpp_.size();
      h_lnbpp_.resize(base + cells);
      HIP_OK(hipMemcpy(h_lnbpp_.data() + base, d_lnbpp.as<void>(), sizeof(double) * cells, hipMemcpyDeviceToHost));
      int64_t c = (int64_t)base;
      for (int k = first; k < first + count; ++k) { h_lnbpp_base_[k] = c; c += (int64_t)(h_plans_[k].L + 1) * (h_plans_[k].W + 1); }
    }
  }
}

// the linear form of K1 (bpp_kernels.hip) on the sequences [first, first + count): no plan of the unfiltered mask
void Engine::bpp_lin_chunk(int first, int count, int64_t cells, double* lnbpp) {
  BppScratch& f = bpp_;
  std::vector<SeqPlan> hp(h_plans_.begin() + first, h_plans_.begin() + first + count);
  int64_t cell_b = 0, pos_b = 0;
  int lmax = 0, wmax = 0, pmax = 0;
  for (SeqPlan& p : hp) {
    p.cell_base = cell_b; p.dmin_base = pos_b;
    cell_b += (int64_t)(p.L + 1) * (p.W + 1); pos_b += p.L + 1;
    lmax = std::max(lmax, (int)p.L); wmax = std::max(wmax, (int)p.W); pmax = std::max(pmax, (int)p.n_canonical);
  }
  f.plans.upload(hp, st_);
  f.xw.alloc(sizeof(double) * 5 * (size_t)cells, true);
  // (the per-sequence sweeps read plane entries outside a sequence's triangle with coefficient 0: they must be finite, so a
  // fresh allocation is cleared once; later loads leave finite values of theirs)
  if (f.band_in.alloc(sizeof(double) * kBppInPlanes * (size_t)cells, true) || !f.planes_finite)
    HIP_OK(hipMemsetAsync(f.band_in.as<void>(), 0, f.band_in.bytes(), st_));
  if (f.band_out.alloc(sizeof(double) * kBppOutPlanes * (size_t)cells, true) || !f.planes_finite)
    HIP_OK(hipMemsetAsync(f.band_out.as<void>(), 0, f.band_out.bytes(), st_));
  f.planes_finite = true;
  for (DevBuf* b : {&f.ext_in, &f.ext_out}) b->alloc(sizeof(double) * (size_t)pos_b, true);
  f.dmin.alloc(sizeof(int16_t) * (size_t)pos_b, true);
  f.plist.alloc(sizeof(int16_t) * (size_t)cells, true);
  f.poff.alloc(sizeof(int32_t) * (size_t)count * (wmax + 2), true);
  BppLinArgs a;
  std::memset(&a, 0, sizeof(a));
  a.et = d_et_.as<EnergyTables>(); a.xet = d_xet_.as<EnergyTables>(); a.cand = f.cand.as<BppCandTable>();
  a.plist = f.plist.as<int16_t>(); a.poff = f.poff.as<int32_t>(); a.poff_stride = wmax + 2;
  a.pmax = pmax;
  a.plans = f.plans.as<SeqPlan>();
  a.seq = d_seq_.as<uint8_t>();
  a.okbits = d_okbits0_.as<uint32_t>();
  a.dmin = f.dmin.as<int16_t>();
  a.xw = f.xw.as<double>(); a.xw_stride = (size_t)cells;
  a.tin = f.band_in.as<double>(); a.tout = f.band_out.as<double>(); a.t_stride = (size_t)cells;
  a.lo_in = f.ext_in.as<double>(); a.lo_out = f.ext_out.as<double>();
  a.no_ene = (flags_ & ELEMDP_NO_ENERGY) ? 1 : 0; a.min_span = min_span(); a.m_min = m_min();
  a.okbits_out = d_okbits1_.as<uint32_t>();
  a.kept = f.kept.as<int32_t>();
  a.log_min_bpp = std::log(min_bpp_);
  a.lnbpp = lnbpp;
  DevBuf d_prof;
  if (getenv("ELEMDP_BPP_PROF")) {
    d_prof.alloc(sizeof(unsigned long long) * 16);
    HIP_OK(hipMemsetAsync(d_prof.as<void>(), 0, sizeof(unsigned long long) * 16, st_));
    a.prof = d_prof.as<unsigned long long>();
  }
  HIP_OK(launch_bpp_lin(a, count, lmax, wmax, st_));
  if (a.prof) {
    unsigned long long h[16];
    HIP_OK(hipMemcpyAsync(h, a.prof, sizeof(h), hipMemcpyDeviceToHost, st_));
    HIP_OK(hipStreamSynchronize(st_));
    static const char* nm[8] = {"stage", "stems", "loops generic", "loops 1xn / bulge", "special shapes", "barrier 1", "unary", "barrier 2"};
    for (int dir = 0; dir < 2; ++dir) {
      unsigned long long tot = 0;
      for (int k = 0; k < 8; ++k) tot += h[dir * 8 + k];
      for (int k = 0; k < 8; ++k)
        fprintf(stderr, "[elemdp bpp prof] %s %-18s %6.2f %%  %.3g cycles per sequence\n", dir ? "out" : "in ", nm[k],
                tot ? 100. * (double)h[dir * 8 + k] / (double)tot : 0., (double)h[dir * 8 + k] / count);
    }
  }
}

// the log-space form of K1 on [first, first + count): the one-state automaton over a plan of the unfiltered mask
void Engine::bpp_log_chunk(int first, int count, int64_t cells, double* lnbpp) {
  BppScratch& f = bpp_;
  PlanSet& tmp = f.plan;   // (one set of buffers for all chunks and loads: DevBuf::alloc keeps what is large enough)
  tmp.inner_only = true;
  build_planset(tmp, first, count, d_okbits0_.as<uint32_t>());
  dbg_lap("load: plan of the unfiltered mask (chunk)");
  // table slots for S = 1: buffers of their own, so that the (much larger) slots of the evaluation pipelines survive a
  // load_batch -- the mini-batch training mode loads before every evaluation
  const size_t band1 = (size_t)kNumBandStates * (Wmax_ + 1) * (Lmax_ + 1), ext1 = (size_t)(Lmax_ + 1);
  f.planes_finite = false;   // (log-space values: log 0 = -inf)
  for (DevBuf* b : {&f.band_in, &f.band_out}) b->alloc(band1 * count * sizeof(double), true);
  for (DevBuf* b : {&f.ext_in, &f.ext_out}) b->alloc(ext1 * count * sizeof(double), true);
  f.tmp.alloc(ext1 * 3 * count * sizeof(double), true);
  const SeqPlan& last = h_plans_.back();   // (nothing writes the weights: cleared when fresh)
  if (f.zero_ws.alloc(sizeof(double) * (size_t)(last.pos_base + last.L + 1)))
    HIP_OK(hipMemsetAsync(f.zero_ws.as<void>(), 0, f.zero_ws.bytes(), st_));
  std::vector<int32_t> order(count);
  std::iota(order.begin(), order.end(), 0);
  std::stable_sort(order.begin(), order.end(), [&](int a2, int b2) { return tmp.h[a2].L > tmp.h[b2].L; });
  f.order.upload(order, st_);
  const int stride = 10;
  f.rows.alloc(sizeof(double) * stride * count);
  TrArgs a;
  std::memset(&a, 0, sizeof(a));
  a.lay = lay0_;
  a.layp = d_lay0_.as<AutomatonLayout>();
  a.ints = d_ints0_.as<int32_t>();
  a.layp_r = a.layp; a.ints_r = a.ints;
  a.params = d_params0_.as<double>();
  a.no_prf = 1;
  a.m_min = m_min();
  a.plans = tmp.d_plans.as<SeqPlan>();
  a.grp = f.order.as<int32_t>();
  a.b.seq = d_seq_.as<uint8_t>(); a.b.ws = f.zero_ws.as<double>(); a.b.unp = d_unp_.as<uint8_t>(); a.b.ndot = nullptr;
  a.okbits = d_okbits0_.as<uint32_t>();
  a.p = tmp.arrays();
  a.band_in = f.band_in.as<double>(); a.band_out = f.band_out.as<double>();
  a.ext_in = f.ext_in.as<double>(); a.ext_out = f.ext_out.as<double>();
  a.band_stride = band1; a.ext_stride = ext1;
  a.tmp = f.tmp.as<double>(); a.tmp_stride = ext1;
  a.seq_out = f.rows.as<double>(); a.out_stride = stride;
  BppOut o;
  o.okbits_out = d_okbits1_.as<uint32_t>();
  o.kept = f.kept.as<int32_t>();
  o.log_min_bpp = std::log(min_bpp_);
  o.lnbpp = lnbpp;
  HIP_OK(hipMemsetAsync(f.rows.as<void>(), 0, sizeof(double) * stride * count, st_));
  const int Lg = tmp.h[order[0]].L;
  HIP_OK(launch_bpp_group(a, o, count, Lg, std::min(Lg, max_span_), st_));
}

// the resident plan of the filtered mask (in d_okbits1_) and the buffers the evaluations size by the batch
void Engine::resident_plan(const uint32_t* mask) {
  const int n = (int)h_plans_.size();
  if (mask != d_okbits1_.as<uint32_t>())
    HIP_OK(hipMemcpyAsync(d_okbits1_.as<void>(), mask, sizeof(uint32_t) * bits_words_, hipMemcpyDeviceToDevice, st_));
  plan_.permuted = true;
  build_planset(plan_, 0, n, d_okbits1_.as<uint32_t>());
  dbg_lap("load: plan of the filtered mask");
  for (int k = 0; k < n; ++k) { plan_.h[k].bpp_eff = h_plans_[k].bpp_eff; plan_.h[k].n_canonical = h_plans_[k].n_canonical; }
  plan_.d_plans.upload(plan_.h, st_);
  h_plans_ = plan_.h;
  d_order_.upload(h_order_, st_);
  std::vector<SeqPlan> sorted(n);
  for (int k = 0; k < n; ++k) { sorted[k] = h_plans_[h_order_[k]]; sorted[k].index = h_order_[k]; }
  d_plans_sorted_.upload(sorted, st_);
  HIP_OK(hipStreamSynchronize(st_));
  d_xwc_.alloc(sizeof(double) * 10 * (size_t)n_cells_total_);
  d_flagged_.alloc(sizeof(int32_t) * ((size_t)n + 1));
  out_stride_ = 6 + 2 * au_.n_theta() + 4;
  d_seq_out_.alloc(sizeof(double) * (size_t)out_stride_ * n);
  // (a ranged evaluation writes the rows of its range only: the rows of a new batch start as zeros, not as what the memory held)
  HIP_OK(hipMemsetAsync(d_seq_out_.as<void>(), 0, sizeof(double) * (size_t)out_stride_ * n, st_));
  slots_.invalidate();   // (a new batch: new Lmax, Wmax)
  ++plan_gen_;
  HIP_OK(hipStreamSynchronize(st_));
  dbg_lap("load: weights / output buffers");
}

// ---- streaming --------------------------------------------------------------------------------------------------------
bool Engine::should_stream(const BatchShape& b) {
  if (inner_) return false;
  if (opt_max_resident_ > 0) return (int)b.plans.size() > opt_max_resident_;
  // resident needs per sequence: plan (terms, CSR offsets, items in four orders, their weights) + its share of the table
  // slots; a batch whose plan alone would take more than half of the free device memory is streamed
  size_t free_b = 0, total_b = 0;
  if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return false;
  const size_t held = slots_.held_bytes(TableSlots::Held::Stream) + d_xwc_.bytes() + d_xwi_.bytes();
  return (double)b.n_cells * 600.0 > 0.5 * (double)(free_b + held);
}

void Engine::stream_setup(const uint8_t* seq, const int32_t* off, const uint8_t* qual, const int32_t* qoff, const char* fix,
                          BatchShape&& b) {
  const int n = (int)b.plans.size();
  h_plans_ = std::move(b.plans);
  st_seq_.assign(seq + off[0], seq + off[n]);
  st_qual_.assign(qual + qoff[0], qual + qoff[n]);
  if (fix) st_fix_.assign(fix + off[0], fix + off[n]); else st_fix_.clear();
  st_slot_budget_ = 0;
  if (opt_max_resident_ > 0) st_chunk_ = opt_max_resident_;
  else {   // two inner engines, each with a fifth of the free memory for its plan
    size_t free_b = 0, total_b = 0;
    HIP_OK(hipMemGetInfo(&free_b, &total_b));
    const double per_seq = (double)b.n_cells / n * 600.0;
    st_chunk_ = (int)std::max(256.0, std::min((double)n, 0.2 * (double)free_b / per_seq));
    st_slot_budget_ = (size_t)(0.2 * (double)free_b);
  }
  st_rows_.clear();
  {
    const int nchunks = (n + st_chunk_ - 1) / st_chunk_;
    st_mask_.assign(nchunks, {});
    st_eff_.assign(nchunks, {});
    st_have_eff_.assign(nchunks, 0);
  }
  // (the buffers of an earlier resident batch would only stand in the way of the inner engines)
  slots_.release();
  d_xwc_.reset(); d_xwi_.reset();
  streaming_ = true;
  n_seq_ = n;
}

void Engine::stream_subs() {
  for (auto& e : sub_) {
    if (e) { e->slot_budget_ = st_slot_budget_; continue; }
    elemdp_model_desc d = desc_;
    d.pattern = desc_pattern_.c_str();
    d.energy_param = desc_has_par_ ? desc_par_.c_str() : nullptr;
    d.device = device_;
    e.reset(new Engine(d));
    e->inner_ = true;
    e->slot_budget_ = st_slot_budget_;
    for (auto const& kv : opt_log_) e->set_option(kv.first, kv.second);
  }
}

void Engine::stream_load_chunk(int k, Engine& e) {
  const int c0 = k * st_chunk_, c1 = std::min(n_seq_, c0 + st_chunk_);
  std::vector<int32_t> off(c1 - c0 + 1), qoff(c1 - c0 + 1);
  for (int t = c0; t <= c1; ++t) { off[t - c0] = h_seq_off_[t] - h_seq_off_[c0]; qoff[t - c0] = h_qual_off_[t] - h_qual_off_[c0]; }
  const size_t s0 = (size_t)(h_seq_off_[c0] - h_seq_off_[0]), q0 = (size_t)(h_qual_off_[c0] - h_qual_off_[0]);
  const bool cached = k < (int)st_mask_.size() && !st_mask_[k].empty();
  if (cached) e.set_filter_preset(st_mask_[k].data(), st_mask_[k].size(), st_eff_[k].data());
  e.load_batch(st_seq_.data() + s0, off.data(), st_qual_.data() + q0, qoff.data(), st_fix_.empty() ? nullptr : st_fix_.data() + s0, c1 - c0,
               st_cons_.empty() ? nullptr : st_cons_.data() + s0);
  if (!cached && k < (int)st_mask_.size() && st_fix_.empty() && !(flags_ & ELEMDP_NO_RSS) && min_bpp_ > 0) e.filter_result(st_mask_[k], st_eff_[k]);
  // the filter's result of the chunk, for elemdp_batch_bpp_eff (chunks write disjoint ranges)
  for (int t = c0; t < c1; ++t) h_plans_[t].bpp_eff = e.h_plans_[t - c0].bpp_eff;
  if (k < (int)st_have_eff_.size()) st_have_eff_[k] = 1;
}

// The streamed form of a call.  checked(): the call's own argument checks and set-up, which come behind the n_param check;
// work(c0, c1, engine): the call on the sequences [c0, c1), the chunk resident on `engine` (the next chunk loads meanwhile),
// and the merge of its results.  last_ms adds up over the chunks.
template <class Checked, class Work> void Engine::stream_call(int n_param_in, Checked checked, Work work) {
  if (n_param_in != n_param()) throw ArgError("n_param mismatch");
  checked();
  last_ms[0] = last_ms[1] = last_ms[2] = 0.;
  stream_subs();
  const int nchunks = (n_seq_ + st_chunk_ - 1) / st_chunk_;
  stream_load_chunk(0, *sub_[0]);
  for (int k = 0; k < nchunks; ++k) {
    Engine& cur = *sub_[k & 1];
    std::exception_ptr err;
    std::thread th;
    if (k + 1 < nchunks)
      th = std::thread([&, k] {
        try { stream_load_chunk(k + 1, *sub_[(k + 1) & 1]); } catch (...) { err = std::current_exception(); }
      });
    try {
      work(k * st_chunk_, std::min(n_seq_, (k + 1) * st_chunk_), cur);
      for (int t = 0; t < 3; ++t) last_ms[t] += cur.last_ms[t];
    } catch (...) {
      if (th.joinable()) th.join();
      throw;
    }
    if (th.joinable()) th.join();
    if (err) std::rethrow_exception(err);
  }
}

// The streamed form of a call that keeps a list (a StagedList or the LoopLists): call(c0, at, engine) is the call on the chunk whose
// first sequence is c0 and whose first position is at; the chunks' lists, one behind the other on the host, become this handle's.
template <class List, class ChunkCall> void Engine::stream_listed(List Engine::*list, int n_param_in, ChunkCall call) {
  typename List::Host host;
  stream_call(n_param_in, [] {}, [&](int c0, int, Engine& e) {
    call(c0, (size_t)(h_seq_off_[c0] - h_seq_off_[0]), e);
    host.append(e.*list, c0);
  });
  (this->*list).adopt(host, st_);
}

void Engine::stream_train(const double* x, int n_param_in, void* partial, bool device_ptr, bool reduce) {
  const int np = partial_len();
  std::vector<double> total(np, 0.), part(np);
  stream_call(n_param_in, [&] {
    // (a range of the batch is evaluated by the resident scaled-linear pipeline only: run_lin_batch; anything else would return
    // sums over the whole batch for it)
    if (opt_eval_count_ > 0 && !(opt_eval_first_ == 0 && opt_eval_count_ == n_seq_))
      throw ArgError("eval_first / eval_count: a streamed batch is evaluated as a whole (load fewer sequences, or raise max_resident)");
    set_theta_from(x);
    st_rows_.assign((size_t)5 * n_seq_, 0.);
  }, [&](int c0, int c1, Engine& e) {
    e.train_partial(x, n_param_in, part.data(), false, false);
    for (int t = 0; t < np; ++t) total[t] += part[t];
    e.seq_stats(st_rows_.data() + (size_t)5 * c0, c1 - c0);
    for (int t = c0; t < c1; ++t) h_plans_[t].bpp_eff = e.plans()[t - c0].bpp_eff;
  });
  if (comm_ && reduce) {
    HIP_OK(hipMemcpyAsync(d_partial_.as<void>(), total.data(), sizeof(double) * np, hipMemcpyHostToDevice, st_));
    RCCL_OK(Rccl::get().AllReduce(d_partial_.as<void>(), d_partial_.as<void>(), (size_t)np, Rccl::kDouble, Rccl::kSum, comm_, st_));
    HIP_OK(hipMemcpyAsync(total.data(), d_partial_.as<void>(), sizeof(double) * np, hipMemcpyDeviceToHost, st_));
    HIP_OK(hipStreamSynchronize(st_));
  }
  if (device_ptr) HIP_OK(hipMemcpy(partial, total.data(), sizeof(double) * np, hipMemcpyHostToDevice));
  else std::memcpy(partial, total.data(), sizeof(double) * np);
}

void Engine::stream_scan(const double* x, int n_param_in, elemdp_scan_out* out) {
  const int nt = au_.n_theta();
  std::vector<double> en(nt, 0.), en_k(nt);
  stream_call(n_param_in, [&] { if (!out) throw ArgError("scan: null output"); }, [&](int c0, int, Engine& e) {
    const size_t so = (size_t)(h_seq_off_[c0] - h_seq_off_[0]), qo = (size_t)(h_qual_off_[c0] - h_qual_off_[0]);
    elemdp_scan_out o = *out;   // the chunk's slices of the caller's arrays (batch offsets)
    if (o.start) o.start += so;
    if (o.inner) o.inner += so;
    if (o.end) o.end += qo;
    if (o.psihat) o.psihat += so;
    if (o.rss) o.rss += so;
    if (o.ys) o.ys += c0;
    if (o.ye) o.ye += c0;
    if (o.exist_prob) o.exist_prob += c0;
    o.en = out->en ? en_k.data() : nullptr;
    e.scan(x, n_param_in, &o);
    if (out->en) for (int t = 0; t < nt; ++t) en[t] += en_k[t];
  });
  if (out->en) std::copy(en.begin(), en.end(), out->en);
}

TrArgs Engine::log_pipeline_args() {
  const int S = au_.S();
  TrArgs a;
  std::memset(&a, 0, sizeof(a));
  a.lay = lay_;
  a.layp = d_lay_.as<AutomatonLayout>();
  a.ints = d_ints_.as<int32_t>();
  a.params = d_params_.as<double>();
  a.no_prf = (flags_ & ELEMDP_NO_PROFILE) ? 1 : 0;
  a.m_min = m_min();
  a.no_rss = (flags_ & ELEMDP_NO_RSS) ? 1 : 0;
  a.first_pass_only = opt_first_pass_only_ ? 1 : 0;
  a.lik_ratio = (flags_ & ELEMDP_LIK_RATIO) ? 1 : 0;
  a.schedule = (opt_schedule_ == 1 && linear_ok_ && !opt_first_pass_only_) ? 1 : 0;
  a.layp_r = d_layr_.as<AutomatonLayout>();
  a.ints_r = d_intsr_.as<int32_t>();
  a.plans = plan_.d_plans.as<SeqPlan>();
  a.b.seq = d_seq_.as<uint8_t>(); a.b.ws = d_ws_.as<double>(); a.b.unp = d_unp_.as<uint8_t>(); a.b.ndot = nullptr;
  a.okbits = d_okbits1_.as<uint32_t>();
  a.p = plan_.arrays();
  a.band_in = slots_.band_in.as<double>(); a.band_out = slots_.band_out.as<double>();
  a.ext_in = slots_.ext_in.as<double>(); a.ext_out = slots_.ext_out.as<double>();
  a.band_stride = (size_t)kNumBandStates * (Wmax_ + 1) * (Lmax_ + 1) * S;
  a.ext_stride = (size_t)(Lmax_ + 1) * S;
  a.tmp = slots_.tmp.as<double>();
  a.tmp_stride = a.ext_stride;
  a.seq_out = d_seq_out_.as<double>();
  a.out_stride = out_stride_;
  return a;
}

void Engine::run_train_batch() {
  if (opt_eval_count_ > 0 && !(opt_eval_first_ == 0 && opt_eval_count_ == n_seq_))
    throw ArgError("eval_first / eval_count: the log-space pipeline (pipeline 3) evaluates the whole batch");
  slots_.ensure(slot_request(au_.S(), 0, false, n_seq_, opt_group_ > 0 ? opt_group_ : 4096), free_device_bytes());
  TrArgs a = log_pipeline_args();
  slots_.set_holds(TableSlots::Holds::DenseLog);
  const int n_slots = slots_.n();
  HIP_OK(hipMemsetAsync(d_seq_out_.as<void>(), 0, sizeof(double) * (size_t)out_stride_ * n_seq_, st_));
  HIP_OK(hipEventRecord(ev_[1], st_));
  for (int g0 = 0; g0 < n_seq_; g0 += n_slots) {
    const int G = std::min(n_slots, n_seq_ - g0);
    a.grp = d_order_.as<int32_t>() + g0;
    const int Lg = h_plans_[h_order_[g0]].L;
    HIP_OK(launch_train_group(a, G, Lg, std::min(Lg, max_span_), st_));
  }
  HIP_OK(hipEventRecord(ev_[2], st_));
  HIP_OK(launch_reduce(d_seq_out_.as<double>(), out_stride_, n_seq_, au_.n_theta(), d_partial_.as<double>(), st_));
}

// The scaled-linear pipeline (lin_kernels.hip); sequences it flags (partition function outside the double range, or a
// structurally empty component) are re-evaluated by the log-space pipeline, which applies the reference's skip rule.
// slots, side buffers and the argument record of the scaled-linear pipeline; returns the balanced group size
bool Engine::poison_tables() {   // true: poisoned (whatever zeros the slots held are gone)
  if (!opt_poison_) return false;
  slots_.clear_zeros();
  for (DevBuf* b : {&slots_.band_in, &slots_.band_out, &slots_.a_in, &slots_.a_out})
    if (b->bytes()) HIP_OK(hipMemsetAsync(b->as<void>(), 0xff, b->bytes(), st_));   // (all-ones bytes: NaN)
  return true;
}

void Engine::lin_weights(int first, int count) {
  LinWeightArgs w;
  const PlanArrays pa = plan_.arrays();
  w.e_stack = pa.e_stack; w.e_ext = pa.e_ext; w.e_ml = pa.e_ml; w.e_close = pa.e_close; w.e_hp = pa.e_hp;
  w.items = pa.items;
  w.items_inner = pa.items_inner; w.items_left = pa.items_left; w.items_right = pa.items_right;
  w.n_cells = (size_t)n_cells_total_; w.n_items = (size_t)plan_.n_items;
  if (count > 0 && count < n_seq_) {   // (records are planned in batch order: the cells of a range of records are contiguous)
    const SeqPlan& p0 = h_plans_[first];
    const SeqPlan& p1 = h_plans_[first + count - 1];
    w.cell_first = (size_t)p0.cell_base;
    w.cell_count = (size_t)(p1.cell_base + (int64_t)(p1.L + 1) * (p1.W + 1) - p0.cell_base);
  }
  w.params = d_params_.as<double>();
  w.xwc = d_xwc_.as<double>(); w.xwi = nullptr;   // (item weights: computed where the records are staged)
  HIP_OK(launch_lin_weights(w, st_));
}

int Engine::prepare_lin(LinArgs& a, bool sched1, bool dense_too, int n_eval, int group_cap, bool own) {
  // schedule 1 sweeps the automaton with the shadow copy of (0,0) (one state more per table row); the scan and schedule 0
  // the plain one.  The slots are sized for the wider row.
  const bool shadow = sched1 && lays_.shadow >= 0;
  const AutomatonLayout& L = shadow ? lays_ : lay_;
  const int S = L.S, Sa = std::max(lay_.S, lays_.S), nap = std::max(lay_.ap_rs, lays_.ap_rs);
  // compact band tables (AutomatonLayout::tab_row doubles per cell); the scan's Viterbi pass sweeps dense tables over the
  // same slots (dense_too)
  const int row = std::max(std::max(lay_.tab_row, lays_.tab_row), dense_too ? kNumBandStates * lay_.S : 0);
  // (an evaluation of a range of the resident batch -- options eval_first / eval_count -- needs slots for that range only)
  const int n_need = n_eval > 0 ? std::min(n_eval, n_seq_) : n_seq_;
  const size_t free_b = free_device_bytes();
  const int group = balanced_group(lin_group_bytes(Lmax_, Wmax_, row, Sa, nap), n_need, group_cap, opt_group_, slot_budget_, free_b,
                                   slots_.held_bytes(TableSlots::Held::Group));
  SlotRequest rq = slot_request(Sa, row, false, n_need, group, nap);
  // a slot per sequence where the call may have it and the batch fits: more slots, the same groups (lock_slots_)
  own_map_ = own && opt_own_slots_ && !inner_ && !dense_too &&
             own_slots_fit(n_need, lin_group_bytes(Lmax_, Wmax_, row, Sa, nap), rq.per_slot(), opt_group_, opt_slots_, slot_budget_, free_b,
                           slots_.held_bytes(TableSlots::Held::Group), slots_.held_bytes(TableSlots::Held::Slots));
  if (own_map_) rq.group = n_need;
  slots_.ensure(rq, free_b);
  if (own_map_ && slots_.n() < n_need) own_map_ = false;   // (the allocation had to shrink after all: the shared mapping)
  lock_slots_ = lockstep_slots(own_map_, group, n_need, slots_.n());
  // (if the allocation had to shrink, rebalance for the slots we got)
  const int gsz = even_groups(n_need, lock_slots_);
  std::memset(&a, 0, sizeof(a));
  a.lay = L;
  a.layp = shadow ? d_lays_.as<AutomatonLayout>() : d_lay_.as<AutomatonLayout>();
  a.ints = shadow ? d_intss_.as<int32_t>() : d_ints_.as<int32_t>();
  a.params = d_params_.as<double>();
  a.lin = shadow ? d_lins_.as<double>() : d_lin_.as<double>();
  // (table-driven unary phases: not under FIX_RSS, whose fixed pairs need not be canonical -- the weight tables are indexed
  // by the pair type)
  a.fast = (opt_fast_ && !(flags_ & ELEMDP_DBG_FIX_RSS)) ? 1 : 0;
  a.no_prf = (flags_ & ELEMDP_NO_PROFILE) ? 1 : 0;
  a.m_min = m_min();
  a.no_rss = (flags_ & ELEMDP_NO_RSS) ? 1 : 0;
  a.lik_ratio = (flags_ & ELEMDP_LIK_RATIO) ? 1 : 0;
  a.ext_block = (flags_ & (ELEMDP_DBG_NO_TURN | ELEMDP_DBG_FIX_RSS)) ? 1 : 4;   // (pairs span >= 5 positions unless one of these)
  a.plans = plan_.d_plans.as<SeqPlan>();
  a.b.seq = d_seq_.as<uint8_t>(); a.b.ws = d_ws_.as<double>(); a.b.unp = d_unp_.as<uint8_t>(); a.b.ndot = nullptr;
  a.ews = d_ews_.as<double>();
  a.okbits = d_okbits1_.as<uint32_t>();
  a.p = plan_.arrays();
  a.xwc = d_xwc_.as<double>(); a.xwc_stride = (size_t)n_cells_total_;
  a.xwi = nullptr; a.xwi_stride = 0;
  a.band_in = slots_.band_in.as<double>(); a.band_out = slots_.band_out.as<double>();
  a.ext_in = slots_.ext_in.as<double>(); a.ext_out = slots_.ext_out.as<double>();
  a.band_stride = slots_.band_stride();
  a.ext_stride = (size_t)(Lmax_ + 1) * S;
  a.zs = slots_.zs.as<double>();
  a.a_in = slots_.a_in.as<double>(); a.a_out = slots_.a_out.as<double>();
  a.a_stride = (size_t)(Wmax_ + 1) * (Lmax_ + 1) * L.ap_rs;
  a.okbits_end = d_okbits_end_.as<uint32_t>();
  a.lmax = Lmax_;
  a.nword_max = nword_max_;
  a.seq_out = d_seq_out_.as<double>();
  a.out_stride = out_stride_;
  a.schedule = sched1 ? 1 : 0;
  a.flagged = d_flagged_.as<int32_t>();
  a.dbg = opt_dbg_;
  a.prof = nullptr;
  if (opt_profile_) {
    d_prof_.alloc(sizeof(long long) * 16 * 64);
    HIP_OK(hipMemsetAsync(d_prof_.as<void>(), 0, sizeof(long long) * 16 * 64, st_));
    a.prof = d_prof_.as<long long>();
  }
  a.n_stage = (L.n_ints <= 4096 && !(opt_dbg_ & 8)) ? L.n_ints : L.n_small;
  return gsz;
}

// One sweep of the scaled-linear pipeline over n sequences in processing order (h_ord / d_ord, plan records d_sorted), cut into
// groups of equal size and dealt round-robin to ns streams, each with its own share of the table slots: the serial parts of a
// group (exterior chains, launch tails) run under the band kernels of another.  work(ak, slot0, G, Lg, Wg, stream) queues one
// group of G sequences (the longest of length Lg, spans up to Wg) with the arguments ak of its slots, the first of which is slot0.
template <class Work>
void Engine::sweep_groups(const LinArgs& a, int n, const int32_t* h_ord, const int32_t* d_ord, const SeqPlan* d_sorted, int gsz,
                          int ns, Work work) {
  // (a slot per sequence: the groups are cut as for the slots of the shared mapping, only their slots differ -- slot_sizing.h)
  const int n_lock = own_map_ ? lock_slots_ : slots_.n();
  const int slots_each = n_lock / ns;
  gsz = stream_group(n, gsz, n_lock, ns);   // every stream the same number of groups
  if (own_map_ && slots_.n() < n) throw StateError("sweep_groups: fewer slots than sequences under the own-slot mapping");
  need_group_streams(ns);
  if (ns > 1) {   // the other streams start behind what st_ has queued so far ...
    HIP_OK(hipEventRecord(gstart_, st_));
    for (int k = 1; k < ns; ++k) HIP_OK(hipStreamWaitEvent(gs_[k], gstart_, 0));
  }
  int gi = 0;
  for (int g0 = 0; g0 < n; g0 += gsz, ++gi) {
    const int k = gi % ns;
    const size_t k0 = group_slot_base(own_map_, g0, k, slots_each);
    LinArgs ak = a;
    ak.band_in += k0 * a.band_stride; ak.band_out += k0 * a.band_stride;
    ak.ext_in += k0 * a.ext_stride; ak.ext_out += k0 * a.ext_stride;
    ak.zs += 4 * k0;
    ak.a_in += k0 * a.a_stride; ak.a_out += k0 * a.a_stride;
    if (a.tr_ext) ak.tr_ext += k0 * a.ext_stride;   // (the scan's trace slots; null elsewhere)
    if (a.trace_stack) ak.trace_stack += k0 * a.trace_stack_stride;
    ak.grp = d_ord + g0;
    ak.plans_slot = d_sorted + g0;
    const int Lg = h_plans_[h_ord[g0]].L;
    work(ak, k0, std::min(gsz, n - g0), Lg, std::min(Lg, max_span_), gs_[k]);
  }
  for (int k = 1; k < ns; ++k) {   // ... and st_ continues behind them
    HIP_OK(hipEventRecord(gdone_[k], gs_[k]));
    HIP_OK(hipStreamWaitEvent(st_, gdone_[k], 0));
  }
}

// Waits for st_ and returns the number of sequences the range check of the scaled-linear pipeline flagged (their indices into
// *list when given).
int Engine::read_flagged(std::vector<int32_t>* list) {
  int32_t n_flagged = 0;
  HIP_OK(hipMemcpyAsync(&n_flagged, d_flagged_.as<void>(), sizeof(int32_t), hipMemcpyDeviceToHost, st_));
  HIP_OK(hipStreamSynchronize(st_));
  if (list) {
    list->resize(n_flagged);
    if (n_flagged) HIP_OK(hipMemcpy(list->data(), d_flagged_.as<int32_t>() + 1, sizeof(int32_t) * n_flagged, hipMemcpyDeviceToHost));
  }
  n_flagged_last_ = n_flagged;
  return n_flagged;
}

// The binding of the zeros a train evaluation with the arguments `a` leaves in the dead entries of the slots (slot_sizing.h); not
// valid where it leaves none a later one could build on: a range of the batch, the shared slot mapping, no mask, the generic
// kernels (which store every entry), a timing experiment.
ZeroBinding Engine::zero_binding(const LinArgs& a, bool sched1, bool ranged) const {
  ZeroBinding z;
  z.valid = own_map_ && !ranged && a.p.useful != nullptr && lin_train_cpb(a) > 0 && !a.no_rss && a.dbg == 0 && !opt_first_pass_only_ &&
            !opt_profile_;
  z.plan = plan_gen_;
  z.slots_gen = slots_.generation(); z.n_slots = slots_.n(); z.band_stride = slots_.band_stride();
  z.own = own_map_ ? 1 : 0; z.n_seq = n_seq_;
  z.S = a.lay.S; z.tab_row = a.lay.tab_row; z.ap_rs = a.lay.ap_rs; z.shadow = a.lay.shadow; z.schedule = sched1 ? 1 : 0;
  // (the options as they are set: what they come to in this evaluation follows from them, the layout and the plan)
  z.useful_mask = opt_useful_mask_ ? 1 : 0; z.loop_prepass = opt_loop_prepass_ ? 1 : 0; z.loop_outside = opt_loop_outside_ ? 1 : 0;
  z.live_blocks = opt_live_blocks_; z.live_span = opt_live_span_; z.deterministic = opt_det_ ? 1 : 0; z.fast = a.fast;
  // (option pair_terms has no field: the words drop terms that are exact zeros and were never added -- no stored entry, dead or
  // live, depends on it, so the zeros of one setting serve the other)
  return z;
}

void Engine::run_lin_batch() {
  const bool sched1 = opt_schedule_ == 1 && linear_ok_ && !opt_first_pass_only_ && lay_.s00 == 0 && lays_.shadow >= 0;
  LinArgs a;
  // the records this evaluation covers (options eval_first / eval_count), in processing order (longest first)
  const bool ranged = opt_eval_count_ > 0 && !(opt_eval_first_ == 0 && opt_eval_count_ == n_seq_);
  const int r0 = ranged ? opt_eval_first_ : 0, n_ev = ranged ? opt_eval_count_ : n_seq_;
  if (r0 < 0 || n_ev <= 0 || r0 + n_ev > n_seq_) throw ArgError("eval_first / eval_count outside the resident batch");
  // (what zeros the slots hold: taken before anything of this evaluation touches them)
  ZeroBinding had = slots_.take_zeros();
  last_zeros_kept_ = false;
  int gsz = prepare_lin(a, sched1, false, n_ev, 8192, !ranged);
  if (opt_useful_mask_) ensure_useful_mask();
  a.p.useful = opt_useful_mask_ ? plan_.useful.as<uint8_t>() : nullptr;   // (the train sweeps only: the scan family sees null)
  // the pair terms go with the mask, where the plan has words (the deterministic mode keeps its walk and with it its order of adds)
  if (opt_useful_mask_ && opt_pair_terms_ && !opt_det_ && plan_.pair_terms_built) {
    a.p.ha_rows = plan_.pair_words.as<unsigned long long>();
    a.p.h1_stems = a.p.ha_rows + (size_t)plan_.n_cells;
  }
  // the loop pre-pass goes with the mask (the launcher drops it where the table-driven form does not run)
  a.loop_pre = (opt_loop_prepass_ && opt_useful_mask_ && loop_prepass_ok(sched1)) ? 1 : 0;
  a.loop_post = (opt_loop_outside_ && opt_useful_mask_ && !opt_det_ && loop_prepass_ok(sched1) && loop_outside_ok(sched1)) ? 1 : 0;
  a.in_d0 = first_inside_diagonal(min_span(), m_min());
  // ... and with it the live-block lists (not in the deterministic mode, whose sums follow the grouping of consecutive cells)
  if (lists_wanted()) {
    const int cpb = lin_train_cpb(a), cap = live_span_for(cpb);
    if (cpb > 0 && ensure_live_blocks(cpb, cap, a.loop_pre != 0 || a.loop_post != 0)) {
      a.p.blocks = plan_.blocks.as<LiveBlock>();
      a.p.blocks_in = plan_.blk_two ? a.p.blocks + (size_t)plan_.n_blocks : nullptr;
      a.live_span = cap;
      a.blk_grid = plan_.h_blk_grid.data();
      a.blk_grid_in = plan_.h_blk_grid_in.data();
    }
  }
  const int32_t* h_ord = h_order_.data();
  const int32_t* d_ord = d_order_.as<int32_t>();
  const SeqPlan* d_sorted = d_plans_sorted_.as<SeqPlan>();
  if (ranged) {
    if (range_key_[0] != r0 || range_key_[1] != n_ev || (int)h_order_r_.size() != n_ev) {
      h_order_r_.clear();
      for (int idx : h_order_) if (idx >= r0 && idx < r0 + n_ev) h_order_r_.push_back(idx);
      std::vector<SeqPlan> sorted(n_ev);
      for (int k = 0; k < n_ev; ++k) { sorted[k] = h_plans_[h_order_r_[k]]; sorted[k].index = h_order_r_[k]; }
      HIP_OK(hipStreamSynchronize(st_));   // (the previous evaluation may still read the arrays)
      d_order_r_.upload(h_order_r_, st_);
      d_plans_sorted_r_.upload(sorted, st_);
      HIP_OK(hipStreamSynchronize(st_));   // (`sorted` is a local)
      range_key_[0] = r0; range_key_[1] = n_ev;
    }
    h_ord = h_order_r_.data();
    d_ord = d_order_r_.as<int32_t>();
    d_sorted = d_plans_sorted_r_.as<SeqPlan>();
    gsz = even_groups(n_ev, lock_slots_);
  }
  HIP_OK(hipMemsetAsync(d_seq_out_.as<double>() + (size_t)r0 * out_stride_, 0, sizeof(double) * (size_t)out_stride_ * n_ev, st_));
  HIP_OK(hipMemsetAsync(d_flagged_.as<void>(), 0, sizeof(int32_t), st_));
  if (opt_det_) {   // deterministic mode: a row of counts per (sequence, block of cells), summed in block order by k4_combine
    a.det = 1;
    a.det_nslot = (Lmax_ + 1 + std::max(1, kThreads / a.lay.S) - 1) / std::max(1, kThreads / a.lay.S) + 1;
    const size_t bytes = sizeof(double) * (size_t)n_seq_ * a.det_nslot * out_stride_;
    d_det_.alloc(bytes);
    HIP_OK(hipMemsetAsync(d_det_.as<void>(), 0, bytes, st_));
    a.det_rows = d_det_.as<double>();
  }
  HIP_OK(hipEventRecord(ev_[1], st_));
  lin_weights(r0, n_ev);
  if (poison_tables()) had = ZeroBinding();
  // the dead entries of these slots still hold the zeros of this very binding: the sweeps store none of them
  const ZeroBinding zb = zero_binding(a, sched1, ranged);
  a.zeros_kept = zeros_match(had, zb) ? 1 : 0;
  // (concurrent groups: not for a handful of sequences, whose tables debug_tables reads, nor under the phase profile)
  const int ns = group_streams(n_ev >= 64 && lock_slots_ >= 64 && !opt_profile_);
  sweep_groups(a, n_ev, h_ord, d_ord, d_sorted, gsz, ns, [&](const LinArgs& ak, size_t, int G, int Lg, int Wg, hipStream_t st) {
    HIP_OK(launch_lin_group(ak, G, Lg, Wg, opt_first_pass_only_, st));
  });
  const int n_flagged = read_flagged();
  if (opt_profile_) {
    std::vector<long long> hp(16 * 64);
    HIP_OK(hipMemcpy(hp.data(), d_prof_.as<void>(), sizeof(long long) * 16 * 64, hipMemcpyDeviceToHost));
    last_prof.assign(16, 0);
    for (size_t k = 0; k < hp.size(); ++k) last_prof[k % 16] += hp[k];
  }
  // (the zeros stand behind an evaluation that stored or kept them, covered every resident sequence and flagged none)
  if (n_flagged == 0) slots_.set_holds(TableSlots::Holds::Linear, a.lay.S, zb.valid ? &zb : nullptr);
  else slots_.set_holds(TableSlots::Holds::DenseLog);
  last_zeros_kept_ = a.zeros_kept != 0;
  if (n_flagged > 0) {
    ensure_sorted_plan();   // (the log-space kernels sum the role lists in list order: kernels.h)
    TrArgs t = log_pipeline_args();
    // (dense tables over the buffers of the compact ones: as many slots as fit, at least one -- TableSlots::ensure)
    const int n_dense = (int)std::max<size_t>(1, std::min<size_t>((size_t)slots_.n(), (slots_.band_stride() * (size_t)slots_.n()) / t.band_stride));
    for (int g0 = 0; g0 < n_flagged; g0 += n_dense) {
      const int G = std::min(n_dense, n_flagged - g0);
      t.grp = d_flagged_.as<int32_t>() + 1 + g0;
      HIP_OK(launch_train_group(t, G, Lmax_, Wmax_, st_));
    }
  }
  HIP_OK(hipEventRecord(ev_[2], st_));
  HIP_OK(launch_reduce(d_seq_out_.as<double>() + (size_t)r0 * out_stride_, out_stride_, n_ev, au_.n_theta(), d_partial_.as<double>(), st_));
}

void Engine::run_train() {
  // pipeline 4 (default): the scaled-linear batch pipeline (lin_kernels.hip), which hands sequences outside the double range to
  // pipeline 3, the log-space batch pipeline (train_kernels.hip).  (Pipeline 2, the fused per-sequence kernel of round 1, is
  // retired for training; its scan schedule stays as the scan's range fallback.)
  if (opt_pipeline_ == 3 || opt_det_) ensure_sorted_plan();
  if (opt_pipeline_ == 3) { run_train_batch(); return; }
  run_lin_batch();
}

void Engine::train_partial(const double* x, int n_param_in, void* partial, bool device_ptr, bool reduce) {
  require_device();
  DeviceGuard dg(device_);
  if (streaming_) { stream_train(x, n_param_in, partial, device_ptr, reduce); return; }
  if (n_seq_ <= 0 && !(comm_ && reduce)) throw StateError("train_eval before load_batch");
  if (n_param_in != n_param()) throw ArgError("n_param mismatch");
  HIP_OK(hipEventRecord(ev_[0], st_));
  last_x_.assign(x, x + n_param_in);
  upload_params(x, lay_, false);
  if (n_seq_ > 0) {
    train_rows_ = false;
    run_train();
    train_rows_ = true;
  } else {   // a rank without a share of the batch: zeros into the all-reduce
    HIP_OK(hipMemsetAsync(d_partial_.as<void>(), 0, sizeof(double) * partial_len(), st_));
    HIP_OK(hipEventRecord(ev_[1], st_));
    HIP_OK(hipEventRecord(ev_[2], st_));
  }
  if (comm_ && reduce)   // sum over the ranks, in place, on the engine's stream (RCCL over xGMI)
    RCCL_OK(Rccl::get().AllReduce(d_partial_.as<void>(), d_partial_.as<void>(), (size_t)partial_len(), Rccl::kDouble, Rccl::kSum, comm_, st_));
  HIP_OK(hipMemcpyAsync(partial, d_partial_.as<void>(), sizeof(double) * partial_len(),
                        device_ptr ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, st_));
  HIP_OK(hipEventRecord(ev_[3], st_));
  HIP_OK(hipStreamSynchronize(st_));
  float ms_all = 0, ms_k = 0;
  HIP_OK(hipEventElapsedTime(&ms_all, ev_[0], ev_[3]));
  HIP_OK(hipEventElapsedTime(&ms_k, ev_[1], ev_[2]));
  last_ms[0] = ms_all;
  last_ms[1] = ms_k;
  last_ms[2] = (opt_pipeline_ == 4) ? (double)n_flagged_last_ : 0.;
}

void Engine::train_finish(const double* r, double* fn, double* gr, double* sum_eff, int32_t* n_skipped) {
  const int nt = au_.n_theta();
  if (fn) *fn = r[0];
  if (sum_eff) *sum_eff = r[1];
  if (n_skipped) *n_skipped = (int32_t)std::llround(r[3]);
  if (!gr) return;
  const double* ENo = r + 4;
  const double* ENx = r + 4 + nt;
  const double* EHo = r + 4 + 2 * nt;
  const double* EHx = EHo + 2;
  int k = 0;
  if (softmax()) {  // chain rule through the row-wise softmax (motif_trainer.hpp:251-261)
    if ((int)theta_.size() != nt) throw StateError("train_finish before any evaluation");
    for (int row = 0; row < au_.n_rows(); ++row) {
      const int o = au_.row_offset(row), w = au_.row_width(row);
      double tot = 0.;
      for (int c = 0; c < w; ++c) tot += ENo[o + c] - ENx[o + c];
      for (int c = 0; c < w; ++c) {
        const double tmp = ENo[o + c] - ENx[o + c];
        const double p = std::exp(theta_[o + c]);
        gr[k++] = (1 - p) * tmp - p * (tot - tmp);
      }
    }
  } else {
    for (int t = 0; t < nt; ++t) gr[k++] = ENo[t] - ENx[t];
  }
  gr[k++] = EHo[0] - EHx[0];
  gr[k++] = EHo[1] - EHx[1];
}

void Engine::seq_stats(double* out, int n) {
  require_device();
  DeviceGuard dg(device_);
  if (n != n_seq_) throw ArgError("seq_stats: n_seq mismatch");
  if (streaming_) {
    if ((int)st_rows_.size() != 5 * n) throw StateError("seq_stats before train_eval");
    std::copy(st_rows_.begin(), st_rows_.end(), out);
    return;
  }
  std::vector<double> h((size_t)out_stride_ * n);
  HIP_OK(hipMemcpy(h.data(), d_seq_out_.as<void>(), sizeof(double) * h.size(), hipMemcpyDeviceToHost));
  for (int k = 0; k < n; ++k)
    for (int c = 0; c < 5; ++c) out[5 * k + c] = h[(size_t)k * out_stride_ + c];
}

// The count columns of the rows as the last train evaluation left them: ENo, ENx [n_theta each], EHo, EHx [2 each].
void Engine::seq_counts(double* out, int n) {
  require_device();
  DeviceGuard dg(device_);
  if (streaming_) throw StateError("seq_counts needs a resident batch (the handle streams this one in chunks)");
  if (n_seq_ <= 0 || !train_rows_) throw StateError("seq_counts before train_eval");
  if (n != n_seq_) throw ArgError("seq_counts: n_seq mismatch");
  const size_t nc = (size_t)out_stride_ - 6;
  std::vector<double> h((size_t)out_stride_ * n);
  HIP_OK(hipMemcpy(h.data(), d_seq_out_.as<void>(), sizeof(double) * h.size(), hipMemcpyDeviceToHost));
  for (int k = 0; k < n; ++k) std::copy(h.begin() + (size_t)k * out_stride_ + 6, h.begin() + (size_t)(k + 1) * out_stride_, out + (size_t)k * nc);
}

void Engine::debug_tables(double* inside, double* outside, double* inside_o, double* outside_o, double* ENo, double* ENx,
                          double* EH) {
  require_device();
  DeviceGuard dg(device_);
  if (n_seq_ != 1 || streaming_) throw StateError("debug_tables needs a resident batch of exactly one sequence");
  auto linear = [&] { return slots_.holds() == TableSlots::Holds::Linear; };
  // (only a train evaluation leaves tables the export can read: not a load, an option that invalidates the slots or a scan-family call)
  if (slots_.n() < 1 || slots_.holds() == TableSlots::Holds::Nothing) throw StateError("debug_tables before train_eval");
  if (linear() && opt_fast_ && !last_x_.empty()) {
    // the table-driven train kernels do not store the planes nothing reads (inside B, outside B and 1): the export repeats the
    // evaluation of the one sequence with the generic kernels, which store every plane
    std::vector<double> part(partial_len());
    ScopedValue<bool> generic(opt_fast_, false);
    train_partial(last_x_.data(), n_param(), part.data(), false, false);
  }
  const SeqPlan& p = h_plans_[0];
  const int Sref = au_.S(), L = p.L, W = p.W;
  // (a schedule-1 evaluation of the linear pipeline leaves tables with one more state per row: the shadow of (0,0))
  const bool lin = linear();
  const int S = lin ? slots_.linear_S() : Sref;
  const AutomatonLayout& TL = (S == lays_.S && lays_.shadow >= 0 && S != Sref) ? lays_ : lay_;
  const std::vector<int32_t>& TI = (&TL == &lays_) ? intss_ : ints_;
  const size_t cells = (size_t)(W + 1) * (L + 1);
  // the scaled-linear pipeline keeps Boltzmann weights times a power-of-two scale (lin_rules.h) in COMPACT tables
  // (TableView::ld / st, dp_rules.h): columns only for the states that are useful in a plane, nothing for cells that are not
  // parsable in it -- the export reads those as 0 -> log 0
  const size_t band = lin ? cells * TL.tab_row : (size_t)7 * cells * S, ext = (size_t)(L + 1) * S;
  auto fetch = [&](const DevBuf& src, size_t cnt) {
    std::vector<double> h(cnt);
    HIP_OK(hipMemcpy(h.data(), src.as<void>(), sizeof(double) * cnt, hipMemcpyDeviceToHost));
    return h;
  };
  std::vector<double> cum(L + 1, 0.);   // log2 of prod_{p<j} psb[base(p)]
  if (lin) for (int t = 0; t < L; ++t) cum[t + 1] = cum[t] + h_lin_[kLinPl2 + h_seq_[p.seq_base + t]];
  const double ln2 = 0.69314718055994530942, NEGINF = -std::numeric_limits<double>::infinity();
  auto ref_id = [&](int s) { return TI[TL.st_ref + s]; };   // tables are exported in the reference's state order
  auto conv = [&](double v, double scale_log2) { return !lin ? v : (v > 0. ? std::log(v) - scale_log2 * ln2 : NEGINF); };
  // liveness of a cell in a plane (is_parsable, energy_model.hpp:289-338) from the pair mask and dmin of the sequence
  std::vector<uint32_t> bits((cells + 31) / 32 + 1, 0u);
  std::vector<int16_t> dmin(L + 1, 0);
  if (lin) {
    HIP_OK(hipMemcpy(bits.data(), d_okbits1_.as<uint32_t>() + p.bits_base, sizeof(uint32_t) * ((cells + 31) / 32), hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(dmin.data(), plan_.arrays().dmin + p.dmin_base, sizeof(int16_t) * (L + 1), hipMemcpyDeviceToHost));
  }
  auto pair_ok = [&](int i, int d) {
    if (i < 0 || d < 0 || d > W || i + d > L) return false;
    const size_t c = (size_t)i * (W + 1) + d;
    return ((bits[c >> 5] >> (c & 31)) & 1u) != 0;
  };
  auto left_ok = [&](int i, int d) { return i >= 0 && d >= 0 && d <= W && i + d <= L && dmin[i] > 0 && d >= dmin[i]; };
  auto cell_live = [&](int e, int d, int i) {
    switch (e) {
      case ST_P: return pair_ok(i, d);
      case ST_E: return i > 0 && d + 2 <= W && pair_ok(i - 1, d + 2);
      case ST_M: return 0 < i && i + d < L && d <= W && m_min() <= d;
      case ST_B: case ST_1: case ST_2: return left_ok(i, d);
      default: return true;
    }
  };
  // value of entry (e, d, i, s) of a fetched table in either layout
  auto tab = [&](const std::vector<double>& t, int e, int d, int i, int s2) {
    if (!lin) return t[(((size_t)e * (W + 1) + d) * (L + 1) + i) * S + s2];
    const int c = TI[TL.tab_cmap + e * S + s2];
    if (c < 0 || !cell_live(e, d, i)) return 0.;
    return t[(size_t)TL.tab_cs[e] * cells + ((size_t)d * (L + 1) + i) * TL.tab_rs[e] + c];
  };
  auto reorder = [&](const std::vector<double>& t, const std::vector<double>* plus2, double* dst, bool outside_tab) {  // -> [i][d][e][s]
    for (int i = 0; i <= L; ++i) for (int d = 0; d <= W; ++d) for (int e = 0; e < 7; ++e) for (int s = 0; s < S; ++s) {
      if (s == TL.shadow) continue;
      double sc = (i + d <= L) ? cum[i + d] - cum[i] : 0.;
      if (outside_tab) sc = cum[L] - sc;
      double v = (i + d <= L) ? tab(t, e, d, i, s) : 0.;
      if (plus2 && e == ST_2 && i + d <= L) v += (*plus2)[((size_t)d * (L + 1) + i) * S + s];
      dst[(((size_t)i * (W + 1) + d) * 7 + e) * Sref + ref_id(s)] = (i + d <= L) ? conv(v, sc) : NEGINF;
    }
  };
  if (inside) reorder(fetch(slots_.band_in, band), nullptr, inside, false);
  if (outside) {
    std::vector<double> to = fetch(slots_.band_out, band), ha;
    if (lin && TL.n_ap > 0 && slots_.a_out.bytes() >= sizeof(double) * cells * TL.ap_rs) {
      // the linear pipeline keeps only the direct part (rules 4a, 3a) of the plane-2 outside values; what arrives through
      // rule 2 is HA(k,l,t) = sum_i sum_{p=(s1,t)} outA(i,l,p) 1(i,k,s1) (lin_rules.h) -- added here for the export
      const int nA = TL.n_ap, nAs = TL.ap_rs;
      const std::vector<double> ti = fetch(slots_.band_in, band), ao = fetch(slots_.a_out, cells * nAs);
      ha.assign(cells * S, 0.);
      for (int d = 0; d <= W; ++d) for (int i = 0; i + d <= L; ++i) for (int q = 0; q < nA; ++q) {
        const int s1 = TI[TL.ap_s1 + q], t = TI[TL.ap_t + q];
        if (!(tab(ti, ST_2, d, i, t) != 0.)) continue;
        double acc = 0.;
        for (int b = 1; d + b <= W && i - b >= 0; ++b)
          if (left_ok(i - b, b))   // 1(i-b, i, .) is parsable; the pair entries of (i-b, d+b) then exist
            acc += ao[((size_t)(d + b) * (L + 1) + (i - b)) * nAs + q] * tab(ti, ST_1, b, i - b, s1);
        ha[((size_t)d * (L + 1) + i) * S + t] += acc;
      }
    }
    reorder(to, ha.empty() ? nullptr : &ha, outside, true);
  }
  if (inside_o) { auto h = fetch(slots_.ext_in, ext); for (int j = 0; j <= L; ++j) for (int s = 0; s < S; ++s) if (s != TL.shadow) inside_o[(size_t)j * Sref + ref_id(s)] = conv(h[(size_t)j * S + s], cum[j]); }
  if (outside_o) { auto h = fetch(slots_.ext_out, ext); for (int j = 0; j <= L; ++j) for (int s = 0; s < S; ++s) if (s != TL.shadow) outside_o[(size_t)j * Sref + ref_id(s)] = conv(h[(size_t)j * S + s], cum[L] - cum[j]); }
  std::vector<double> o = fetch(d_seq_out_, out_stride_);
  const int nt = au_.n_theta();
  if (ENo) std::copy(o.begin() + 6, o.begin() + 6 + nt, ENo);
  if (ENx) std::copy(o.begin() + 6 + nt, o.begin() + 6 + 2 * nt, ENx);
  if (EH) std::copy(o.begin() + 6 + 2 * nt, o.begin() + 6 + 2 * nt + 4, EH);
}

void Engine::batch_pairs(int idx, uint8_t* kept, double* lnbpp, int cap) {
  require_device();
  DeviceGuard dg(device_);
  if (streaming_) throw StateError("batch_pairs needs a resident batch (the handle streams this one in chunks)");
  if (idx < 0 || idx >= n_seq_) throw ArgError("batch_pairs: bad sequence index");
  const SeqPlan& p = h_plans_[idx];
  const int nc = (p.L + 1) * (p.W + 1);
  if (cap < nc) throw ArgError("batch_pairs: buffer too small");
  const int nword = (nc + 31) / 32;
  std::vector<uint32_t> w(nword);
  HIP_OK(hipMemcpy(w.data(), d_okbits1_.as<uint32_t>() + p.bits_base, sizeof(uint32_t) * nword, hipMemcpyDeviceToHost));
  for (int c = 0; c < nc; ++c) kept[c] = (w[c >> 5] >> (c & 31)) & 1u;
  if (lnbpp) {
    if (h_lnbpp_base_.empty()) throw StateError("ln BPP was not kept (set option keep_lnbpp before load_batch)");
    std::vector<uint32_t> w0(nword);
    HIP_OK(hipMemcpy(w0.data(), d_okbits0_.as<uint32_t>() + p.bits_base, sizeof(uint32_t) * nword, hipMemcpyDeviceToHost));
    for (int c = 0; c < nc; ++c)
      lnbpp[c] = ((w0[c >> 5] >> (c & 31)) & 1u) ? h_lnbpp_[h_lnbpp_base_[idx] + c] : -std::numeric_limits<double>::infinity();
  }
}

// Does a train evaluation take the plan's lists (where the model's kernels take any)?  Not without the mask, and not in the
// deterministic mode, whose sums follow the grouping of consecutive cells.
bool Engine::lists_wanted() const { return opt_useful_mask_ && opt_live_blocks_ && !opt_det_; }
// can the loop pre-pass serve the automaton a train evaluation sweeps (the one with the shadow state under schedule 1)?
bool Engine::loop_outside_ok(bool sched1) const {
  const bool shadow = sched1 && lays_.shadow >= 0;
  return lin_loop_outside_ok(shadow ? lays_ : lay_, shadow ? intss_.data() : ints_.data());
}
bool Engine::loop_prepass_ok(bool sched1) const {
  const bool shadow = sched1 && lays_.shadow >= 0;
  return lin_loop_prepass_ok(shadow ? lays_ : lay_, shadow ? intss_.data() : ints_.data(), min_span());
}

// the span a block of `cpb` live cells may cover: option live_span, or the default
int Engine::live_span_for(int cpb) const {
  // (never below cpb: a block of cpb consecutive live cells must fit, and only then is ceil(ncell / cpb) blocks enough -- a model
  // with more cells per block than the option asks for takes cpb)
  return std::max(cpb, opt_live_span_ > 0 ? opt_live_span_ : std::min(kLiveSpanDefault, lin_live_span_max()));
}

// The lists of sequence idx for the cells per block and the span of the current options (built here if no evaluation has):
// counts[d] blocks of diagonal d at records + d * stride (16-byte LiveBlock records); cpb_cap = {cells per block, span};
// taken[d] (may be null) = 1 where a train evaluation of the current options sweeps diagonal d from its list.
// inside: the second set (the lists of the inside sweep behind the loop pre-pass, from the bytes without UB_L) and its own choice.
void Engine::live_blocks(int idx, int32_t* counts, void* records, int stride, int32_t* cpb_cap, int32_t* taken, bool inside) {
  require_device();
  DeviceGuard dg(device_);
  if (streaming_) throw StateError("live_blocks needs a resident batch (the handle streams this one in chunks)");
  if (idx < 0 || idx >= n_seq_) throw ArgError("live_blocks: bad sequence index");
  const SeqPlan& p = h_plans_[idx];
  const bool sched1 = opt_schedule_ == 1 && linear_ok_ && !opt_first_pass_only_ && lay_.s00 == 0 && lays_.shadow >= 0;
  LinArgs a;
  prepare_lin(a, sched1, false, n_seq_);
  const int cpb = lin_train_cpb(a);
  if (cpb <= 0) throw StateError("live_blocks: the train sweeps of this model do not take lists");
  const int cap = live_span_for(cpb);
  if (stride < live_blocks_slots(p.L)) throw ArgError("live_blocks: stride too small");
  if (!ensure_live_blocks(cpb, cap, inside)) throw StateError("live_blocks: no lists for this batch");
  HIP_OK(hipStreamSynchronize(st_));
  std::vector<LiveBlock> h((size_t)live_blocks_records(p.L, p.W));
  HIP_OK(hipMemcpy(h.data(), plan_.blocks.as<LiveBlock>() + (inside ? (size_t)plan_.n_blocks : 0) + p.blk_base, sizeof(LiveBlock) * h.size(), hipMemcpyDeviceToHost));
  LiveBlock* out = static_cast<LiveBlock*>(records);
  for (int d = 0; d <= p.W; ++d) {
    counts[d] = h[d].count;
    for (int b = 0; b < counts[d]; ++b) out[(size_t)d * stride + b] = h[(size_t)live_blocks_at(p.L, p.W, d) + b];
  }
  cpb_cap[0] = cpb; cpb_cap[1] = cap;
  // which diagonals a train evaluation of the current options sweeps from these lists
  // (the inside set: only behind the pre-pass, and not below the first diagonal that has an entry outside the L plane)
  const bool want = lists_wanted() && (!inside || (opt_loop_prepass_ && loop_prepass_ok(sched1)));
  const std::vector<int32_t>& grid = inside ? plan_.h_blk_grid_in : plan_.h_blk_grid;
  const int d0 = inside ? first_inside_diagonal(min_span(), m_min()) : 0;
  if (taken) for (int d = 0; d <= p.W; ++d) taken[d] = (want && d >= d0 && grid[d] >= 0) ? 1 : 0;
}

void Engine::useful_mask(int idx, uint8_t* mask, int cap) {
  require_device();
  DeviceGuard dg(device_);
  if (streaming_) throw StateError("useful_mask needs a resident batch (the handle streams this one in chunks)");
  if (idx < 0 || idx >= n_seq_) throw ArgError("useful_mask: bad sequence index");
  const SeqPlan& p = h_plans_[idx];
  const int nc = (p.L + 1) * (p.W + 1);
  if (cap < nc) throw ArgError("useful_mask: buffer too small");
  ensure_useful_mask();
  HIP_OK(hipStreamSynchronize(st_));
  HIP_OK(hipMemcpy(mask, plan_.useful.as<uint8_t>() + p.cell_base, nc, hipMemcpyDeviceToHost));
}

// The pair-term words of sequence idx (built with the mask if no evaluation has): (W+1) * (L+1) words each, [d][i].
void Engine::pair_terms(int idx, uint64_t* ha, uint64_t* h1, int cap) {
  require_device();
  DeviceGuard dg(device_);
  if (streaming_) throw StateError("pair_terms needs a resident batch (the handle streams this one in chunks)");
  if (idx < 0 || idx >= n_seq_) throw ArgError("pair_terms: bad sequence index");
  const SeqPlan& p = h_plans_[idx];
  const int nc = (p.L + 1) * (p.W + 1);
  if (cap < nc) throw ArgError("pair_terms: buffer too small");
  ensure_useful_mask();
  if (!plan_.pair_terms_built) throw StateError("pair_terms: no words for this plan (a span above 64, or the mask of all ones)");
  HIP_OK(hipStreamSynchronize(st_));
  const unsigned long long* w = plan_.pair_words.as<unsigned long long>();
  HIP_OK(hipMemcpy(ha, w + p.cell_base, sizeof(uint64_t) * nc, hipMemcpyDeviceToHost));
  HIP_OK(hipMemcpy(h1, w + (size_t)plan_.n_cells + p.cell_base, sizeof(uint64_t) * nc, hipMemcpyDeviceToHost));
}

// The scaled-linear sum passes of a scan (and the first one of pair_posteriors): table slots, cleared outputs, weights.  A scan
// is one pass: 1 024 sequences per group run within 4 % of the largest groups and need a third of the table memory (an
// evaluation loop that already holds larger groups keeps them).  Returns the balanced group size.
int Engine::prepare_scan(LinArgs& a, const ScanPos& pos) {
  const int n = n_seq_;
  const size_t n_seqpos = (size_t)h_seq_off_[n];
  const int gsz = prepare_lin(a, false, true, 0, std::max(1024, slots_.n()));
  a.scan = 1;
  a.ys = pos.ys.as<int32_t>(); a.ye = pos.ye.as<int32_t>();
  a.pos_start = pos.start.as<double>(); a.pos_inner = pos.inner.as<double>(); a.pos_end = pos.end.as<double>();
  a.exist = pos.exist.as<double>();
  HIP_OK(hipMemsetAsync(pos.start.as<void>(), 0, 8 * n_seqpos, st_));
  HIP_OK(hipMemsetAsync(pos.inner.as<void>(), 0, 8 * n_seqpos, st_));
  HIP_OK(hipMemsetAsync(pos.end.as<void>(), 0, 8 * (n_seqpos + n), st_));
  HIP_OK(hipMemsetAsync(pos.ys.as<void>(), 0, 4 * (size_t)n, st_));
  HIP_OK(hipMemsetAsync(pos.ye.as<void>(), 0, 4 * (size_t)n, st_));
  HIP_OK(hipMemsetAsync(d_seq_out_.as<void>(), 0, sizeof(double) * (size_t)out_stride_ * n, st_));
  HIP_OK(hipMemsetAsync(d_flagged_.as<void>(), 0, sizeof(int32_t), st_));
  lin_weights();
  poison_tables();
  return gsz;
}

// The fused scan kernel (the log-space form) and its block count.  After the scaled-linear sum passes it reuses their table and
// trace slots; otherwise (pipeline 3) it gets table slots with trace tables, which the train pipelines do not reuse:
// scan_log_form marks them (Holds::Trace) when done.
DpArgs Engine::log_scan_args(bool sums_on_batch, int* n_blocks) {
  const int n = n_seq_, S = au_.S();
  if (sums_on_batch) {
    *n_blocks = std::min(std::min(slots_.n(), 2 * n_cu_), n);
  } else {
    slots_.ensure(slot_request(S, 0, true, n), free_device_bytes());
    *n_blocks = std::min(slots_.n(), n);
  }
  DpArgs d = base_args(lay_, d_ints_.as<int32_t>(), d_params_.as<double>(), plan_, d_okbits1_.as<uint32_t>(), S);
  d.lds = lds_layout(lay_, Lmax_, nword_max_, true);
  return d;
}

void Engine::require_resident(const char* what, int n_param_in) {
  if (n_seq_ <= 0) throw StateError(std::string(what) + " before load_batch");
  if (n_param_in != n_param()) throw ArgError("n_param mismatch");
  train_rows_ = false;   // (the scan family writes rows of its own into d_seq_out_)
}

// Sequences per launch of the log-space form of a call with per-slot scratch: what the table slots hold behind the sum passes,
// else (pipeline 3) what the scratch of the call is sized for.
int Engine::log_chunk(int n_blocks, int n_log) const {
  return std::min(n_log, opt_pipeline_ == 4 ? slots_.n() : std::max(n_blocks, 1024));
}

// The per-slot scratch of a scan-family call: `stride` elements of T per slot in b, one slot per table slot behind prepare_scan
// (slots_.n(), known in the fill of scan_sums at the earliest), one per sequence of a log_chunk under pipeline 3 -- the one sizing
// rule, scratch_slots_, which scan_sums and scan_log_form set.  Returns the scratch of slot slot0.  A call sizes its scratch in its
// fill, before anything is queued, by pointing its argument record at slot 0; the same request again keeps the buffer
// (DevBuf::alloc), so a group asks with its own slot0.
template <class T> T* Engine::slot_scratch(DevBuf& b, size_t stride, size_t slot0) {
  b.alloc(sizeof(T) * stride * std::max<size_t>(scratch_slots_, 1));
  return b.as<T>() + slot0 * stride;
}

// The pair reduction's arguments (pair_posteriors, context_profile).  pair_batch_args: its view of the batch -- plan, mask and rows --
// which both forms of a call need.  pair_plane_fields: behind prepare_scan, with the arguments `a` of the sum pass, where the P plane
// lies in a compact table slot (the scaled-linear form only).
PairArgs Engine::pair_batch_args() const {
  PairArgs pa;
  std::memset(&pa, 0, sizeof(pa));
  pa.plans = plan_.d_plans.as<SeqPlan>();
  pa.okbits = d_okbits1_.as<uint32_t>();
  pa.seq_out = d_seq_out_.as<double>(); pa.out_stride = out_stride_;
  return pa;
}

void Engine::pair_plane_fields(PairArgs& pa, const LinArgs& a) const {
  // the P plane's columns of the real states are 0 .. ncol-1: Automaton::flatten numbers a plane's columns in state order,
  // and a shadow state comes last
  int ncol = 0;
  for (int s = 0; s < a.lay.S; ++s) {
    const int c = ints_[a.lay.tab_cmap + ST_P * a.lay.S + s];
    if (s == a.lay.shadow || c < 0) continue;
    if (c != ncol) throw std::logic_error("pair reduction: the P plane's columns are not in state order");
    ++ncol;
  }
  pa.p_cs = a.lay.tab_cs[ST_P]; pa.p_rs = a.lay.tab_rs[ST_P];
  pa.ncol = ncol;
  pa.band_stride = a.band_stride;
  pa.skip_flagged = 1;
}

// The scaled-linear form of a scan-family call (pipeline 4): the scan's first sum pass on the groups, slots and streams of
// Engine::scan.  fill(a) adds the call's fields to the argument record and sizes the call's per-slot scratch (slots_.n() is known
// only behind prepare_scan); group(ak, slot0, G, Lg, Wg, stream) queues a group's work as for sweep_groups.  Waits for the device
// and returns the number of sequences the range check flagged (their indices into *flagged when given): those are left to
// scan_log_form.
template <class Fill, class Group>
int Engine::scan_sums(const ScanPos& pos, Fill fill, Group group, std::vector<int32_t>* flagged) {
  LinArgs a;
  const int gsz = prepare_scan(a, pos);
  scratch_slots_ = (size_t)slots_.n();
  fill(a);
  const int ns = group_streams(n_seq_ >= 128 && slots_.n() >= 128);
  sweep_groups(a, n_seq_, h_order_.data(), d_order_.as<int32_t>(), d_plans_sorted_.as<SeqPlan>(), gsz, ns, group);
  dbg_lap("scan sums: launches queued");
  const int n_flagged = read_flagged(flagged);
  dbg_lap("scan sums: device done");
  slots_.set_holds(TableSlots::Holds::Nothing);   // (not what a train evaluation leaves: debug_tables refuses)
  return n_flagged;
}

// The log-space form of a scan-family call: the fused scan kernel on the n_flagged sequences the range check of scan_sums flagged
// (listed behind the count in d_flagged_), or -- pipeline 3, no sum passes on the batch -- on every sequence in processing order.
// fill(d, n_blocks, n_log) sets the call's fields of the kernel's arguments, sizes the call's scratch and returns the most
// sequences one launch may take; behind(idx, C) queues the call's work on the C sequences idx[0 .. C) of a launch behind it.
template <class Fill, class Behind>
void Engine::scan_log_form(bool sums_on_batch, int n_flagged, Fill fill, Behind behind) {
  const int n_log = sums_on_batch ? n_flagged : n_seq_;
  if (n_log > 0) {
    int n_blocks;
    DpArgs d = log_scan_args(sums_on_batch, &n_blocks);
    if (!sums_on_batch) scratch_slots_ = (size_t)log_chunk(n_blocks, n_log);
    const int chunk = fill(d, n_blocks, n_log);
    const int32_t* list = sums_on_batch ? d_flagged_.as<int32_t>() + 1 : d_order_.as<int32_t>();
    for (int c0 = 0; c0 < n_log; c0 += chunk) {
      const int C = std::min(chunk, n_log - c0);
      d.order = list + c0;
      d.n_seq = C;
      HIP_OK(hipMemsetAsync(d_counter_.as<void>(), 0, sizeof(int32_t), st_));
      HIP_OK(launch_dp(DP_SCAN, d, std::min(n_blocks, C), st_));
      behind(list + c0, C);
    }
  }
  if (!sums_on_batch) slots_.set_holds(TableSlots::Holds::Trace);   // the slots of log_scan_args are not reused by the train pipelines
}

// Both forms of a scan-family call, queued behind ev_[1]: the sum passes on the batch under pipeline 4 (scan_sums: fill, group),
// then the log-space form for what they flagged, or for the whole batch otherwise (scan_log_form: log_fill, behind).  Returns the
// number of sequences the range check flagged.
// in_world: the call honours option world -- both argument records carry the world, the group work starts with
// launch_lin_world_group, and a world other than the mixture takes the range check over all three Z (LinArgs::range_all).
template <class Fill, class Group, class LogFill, class Behind>
int Engine::scan_both_forms(const ScanPos& pos, Fill fill, Group group, LogFill log_fill, Behind behind, bool in_world) {
  const bool sums_on_batch = opt_pipeline_ == 4;
  const int world = in_world ? opt_world_ : 0;
  const int n_flagged = sums_on_batch ? scan_sums(pos, [&](LinArgs& a) {
    fill(a);
    a.world = world;
    if (world != 0) a.range_all = 1;
  }, group) : 0;
  scan_log_form(sums_on_batch, n_flagged, [&](DpArgs& d, int n_blocks, int n_log) {
    const int chunk = log_fill(d, n_blocks, n_log);
    d.smp.world = world;      // (behind the fill: the sampler's fill copies its whole record)
    return chunk;
  }, behind);
  return n_flagged;
}

// The end of a scan-family call and its times (elemdp_last_timing): ev_[1] .. ev_[2] is the whole call, ev_[1] .. ev_[3] its
// kernels.  copy_out() queues on st_ what the call counts as its way out -- asynchronous copies to the host, the scatter of a list
// -- between ev_[3] and ev_[2].  Without one (scan, sample_structures) there is no ev_[3] and both times are the same; what such a
// call hands out it fetches with blocking copies behind this, outside the timed window.
void Engine::finish_call(int n_flagged) {
  HIP_OK(hipEventRecord(ev_[2], st_));
  HIP_OK(hipStreamSynchronize(st_));
  float ms = 0;
  HIP_OK(hipEventElapsedTime(&ms, ev_[1], ev_[2]));
  last_ms[0] = last_ms[1] = ms;
  last_ms[2] = (double)n_flagged;
}
template <class Copy> void Engine::finish_call(int n_flagged, Copy copy_out) {
  HIP_OK(hipEventRecord(ev_[3], st_));
  copy_out();
  finish_call(n_flagged);
  float ms_dp = 0;
  HIP_OK(hipEventElapsedTime(&ms_dp, ev_[1], ev_[3]));
  last_ms[1] = ms_dp;
}

void Engine::scan(const double* x, int n_param_in, elemdp_scan_out* out) {
  require_device();
  DeviceGuard dg(device_);
  if (streaming_) { stream_scan(x, n_param_in, out); return; }
  require_resident("scan", n_param_in);
  // (--no-rss: load_batch cleared the pair mask, so every sweep reduces to the exterior chain = the profile-HMM
  // forward / backward / Viterbi of motif_model.hpp:171-206 under the scanner functors, motif_scanner.hpp:186-214)
  if (!out) throw ArgError("scan: null output");
  upload_params(x, lay_, false);
  const int nt = au_.n_theta(), n = n_seq_, S = au_.S();
  const size_t n_seqpos = (size_t)h_seq_off_[n], n_pos = n_seqpos + n;
  ScanPos pos(n_seqpos, n);
  DevBuf d_psi, d_rss, d_en;
  d_psi.alloc(4 * n_seqpos); d_rss.alloc(n_seqpos); d_en.alloc(8 * (size_t)n * (nt + 1));
  HIP_OK(hipEventRecord(ev_[1], st_));
  const int stack_stride = trace_stack_stride(Lmax_);
  auto scan_fields = [&](DpArgs& d) {   // what the fused kernel reads and writes of a scan
    d.tr_ext = slots_.tr_ext.as<TraceRec>();
    d.trace_stack = slots_.tr_stack.as<int32_t>();
    d.trace_stack_stride = stack_stride;
    d.sc_start = pos.start.as<double>(); d.sc_end = pos.end.as<double>(); d.sc_inner = pos.inner.as<double>();
    d.sc_psihat = d_psi.as<int32_t>(); d.sc_rss = d_rss.as<char>();
    d.sc_ys = pos.ys.as<int32_t>(); d.sc_ye = pos.ye.as<int32_t>(); d.sc_exist = pos.exist.as<double>(); d.sc_en = d_en.as<double>();
  };
  // ---- K4 / K5 (the four sum passes, motif_scanner.hpp:186-202) on the scaled-linear batch pipeline
  std::vector<int32_t> flagged;
  const bool sums_on_batch = opt_pipeline_ == 4;
  if (sums_on_batch) {
    dbg_lap("scan: start");
    const bool cyk_on_batch = !(opt_dbg_ & 64);
    scan_sums(pos, [&](LinArgs& a) {
      // trace records of the Viterbi pass: the exterior chain's rows and the traceback stack per table slot (the band targets keep
      // none: scan_rules.h, cyk_retrace)
      slots_.ensure_trace();
      dbg_lap("scan: trace slots");
      a.tr_ext = slots_.tr_ext.as<TraceRec>();
      a.trace_stack = slots_.tr_stack.as<int32_t>(); a.trace_stack_stride = stack_stride;
      a.sc_psihat = d_psi.as<int32_t>(); a.sc_rss = d_rss.as<char>();
    }, [&](const LinArgs& ak, size_t, int G, int Lg, int Wg, hipStream_t st) {
      HIP_OK(launch_lin_scan_group(ak, G, Lg, Wg, SCAN_PASS_START, st));
      HIP_OK(launch_lin_scan_group(ak, G, Lg, Wg, SCAN_PASS_END, st));
      if (cyk_on_batch) HIP_OK(launch_cyk_group(ak, G, Lg, Wg, st));   // K6 on the same table slots
    }, &flagged);
    if (!cyk_on_batch) {   // K6 (Viterbi parse + traceback) of the whole batch on the fused kernel
      int n_blocks;
      DpArgs d = log_scan_args(true, &n_blocks);
      scan_fields(d);
      d.order = d_order_.as<int32_t>();
      d.cyk_only = 1;
      HIP_OK(hipMemsetAsync(d_counter_.as<void>(), 0, sizeof(int32_t), st_));
      HIP_OK(launch_dp(DP_SCAN, d, n_blocks, st_));
    }
  }
  // ---- the fused kernel runs the whole schedule, K6 included, for the sequences the linear passes flagged (range check) and
  // for pipeline != 4
  scan_log_form(sums_on_batch, (int)flagged.size(), [&](DpArgs& d, int, int n_log) { scan_fields(d); return n_log; },
                [](const int32_t*, int) {});
  finish_call((int)flagged.size());
  auto get = [&](void* dst, const DevBuf& src, size_t bytes) { if (dst) HIP_OK(hipMemcpy(dst, src.as<void>(), bytes, hipMemcpyDeviceToHost)); };
  get(out->start, pos.start, 8 * n_seqpos);
  get(out->inner, pos.inner, 8 * n_seqpos);
  get(out->end, pos.end, 8 * n_pos);
  get(out->psihat, d_psi, 4 * n_seqpos);
  get(out->rss, d_rss, n_seqpos);
  get(out->ys, pos.ys, 4 * n);
  get(out->ye, pos.ye, 4 * n);
  get(out->exist_prob, pos.exist, 8 * n);
  if (out->en) {  // E[N] summed over the batch in input order (motif_scanner.hpp:253-259)
    for (int t = 0; t < nt; ++t) out->en[t] = 0.;
    std::vector<char> is_flagged(n, 0);
    for (int k : flagged) is_flagged[k] = 1;
    std::vector<double> h((size_t)n * nt), rows;
    if (!sums_on_batch || !flagged.empty()) HIP_OK(hipMemcpy(h.data(), d_en.as<void>(), 8 * h.size(), hipMemcpyDeviceToHost));
    if (sums_on_batch) {
      rows.resize((size_t)out_stride_ * n);
      HIP_OK(hipMemcpy(rows.data(), d_seq_out_.as<void>(), sizeof(double) * rows.size(), hipMemcpyDeviceToHost));
    }
    for (int k = 0; k < n; ++k)
      for (int t = 0; t < nt; ++t)
        out->en[t] += (sums_on_batch && !is_flagged[k]) ? rows[(size_t)k * out_stride_ + 6 + t] : h[(size_t)k * nt + t];
  }
}


// ---- base-pair posteriors under the motif model (pair_rules.h).  The scan's first sum pass per group, the pair
// reduction on the group's table slots right behind it (before the next group of the stream reuses them), the log-space form --
// the fused scan kernel up to its first outside pass -- for the sequences that leave the double range and under pipeline 3, then
// the batch list in (sequence, i, j) order: prefix over the per-sequence counts, scatter out of the staging ranges.
void Engine::pair_posteriors(const double* x, int n_param_in, double min_prob, int64_t* n_pairs, double* unpaired,
                             const MeaOut* mea) {
  require_device();
  DeviceGuard dg(device_);
  if (!n_pairs) throw ArgError("pair_posteriors: null n_pairs");
  if (!(min_prob >= 0.)) throw ArgError("pair_posteriors: min_prob must be >= 0");
  if (mea && !(std::isfinite(mea->gamma) && mea->gamma > 0.)) throw ArgError("pair_mea: gamma must be finite and > 0");
  pairs_.invalidate();
  if (streaming_) { stream_pairs(x, n_param_in, min_prob, unpaired, mea); *n_pairs = pairs_.count(); return; }
  require_resident("pair_posteriors", n_param_in);
  upload_params(x, lay_, false);
  const int n = n_seq_;
  const size_t n_seqpos = (size_t)h_seq_off_[n];
  const size_t pcells = (size_t)(Lmax_ + 1) * (Wmax_ + 1);   // P(i, d) of one table slot
  ScanPos pos(n_seqpos, n);
  d_pr_unp_.alloc(8 * n_seqpos);
  HIP_OK(hipEventRecord(ev_[1], st_));
  const StagedList::Staging sl = pairs_.begin(plan_.d_plans.as<SeqPlan>(), d_okbits1_.as<uint32_t>(), n, 1, st_);
  PairArgs pa = pair_batch_args();
  pa.p_stride = pcells;
  pa.min_prob = min_prob;
  pa.unpaired = d_pr_unp_.as<double>();
  pa.koff = sl.koff; pa.cnt = sl.cnt;
  pa.st_i = sl.st_i; pa.st_j = sl.st_j; pa.st_p = sl.st_v[0];
  // per slot: P(i, d); MEA: the M table and the choices next to it, the chain's choices after the table's (L+1)(W+1)
  const size_t mea_ch_stride = pcells + (size_t)Lmax_ + 1;
  auto at_slot = [&](PairArgs& pk, size_t slot0) {
    pk.P = slot_scratch<double>(d_pr_P_, pcells, slot0);
    if (!mea) return;
    pk.mea_M = slot_scratch<double>(d_mea_M_, pcells, slot0);
    pk.mea_ch = slot_scratch<int32_t>(d_mea_ch_, mea_ch_stride, slot0);
  };
  if (mea) {
    d_mea_s_.alloc(n_seqpos); d_mea_sc_.alloc(8 * (size_t)n);
    pa.mea_gamma2 = 2. * mea->gamma;
    pa.mea_ch_stride = mea_ch_stride;
    pa.mea_s = d_mea_s_.as<char>(); pa.mea_score = d_mea_sc_.as<double>();
  }
  const int n_flagged = scan_both_forms(pos, [&](LinArgs& a) {
    at_slot(pa, 0);
    pair_plane_fields(pa, a);
  }, [&](const LinArgs& ak, size_t slot0, int G, int Lg, int Wg, hipStream_t st) {
    HIP_OK(launch_lin_world_group(ak, G, Lg, Wg, st));
    PairArgs pk = pa;
    pk.idx = ak.grp;
    pk.band_in = ak.band_in; pk.band_out = ak.band_out; pk.zs = ak.zs + ak.world;
    at_slot(pk, slot0);
    HIP_OK(launch_pair_cells(pk, G, (Lg + 1) * (Wg + 1), st));
    HIP_OK(launch_pair_seq(pk, G, st));
    if (mea) HIP_OK(launch_pair_mea(pk, G, Wmax_, st));
  },
  // ---- the log-space form, in chunks of at most as many sequences as the table slots hold (the P scratch is bounded by the chunk)
  [&](DpArgs& d, int n_blocks, int n_log) {
    at_slot(pa, 0);
    d.pair_p = pa.P;
    d.pair_stride = pcells;
    return log_chunk(n_blocks, n_log);
  }, [&](const int32_t* idx, int C) {
    PairArgs pk = pa;
    pk.idx = idx;
    pk.skip_flagged = 0;
    HIP_OK(launch_pair_seq(pk, C, st_));
    if (mea) HIP_OK(launch_pair_mea(pk, C, Wmax_, st_));
  });
  finish_call(n_flagged, [&] { *n_pairs = pairs_.finish(st_); });   // the list in (sequence, i, j) order
  if (unpaired) HIP_OK(hipMemcpy(unpaired, d_pr_unp_.as<void>(), 8 * n_seqpos, hipMemcpyDeviceToHost));
  if (mea && mea->structure) HIP_OK(hipMemcpy(mea->structure, d_mea_s_.as<void>(), n_seqpos, hipMemcpyDeviceToHost));
  if (mea && mea->score) HIP_OK(hipMemcpy(mea->score, d_mea_sc_.as<void>(), 8 * (size_t)n, hipMemcpyDeviceToHost));
}

void Engine::stream_pairs(const double* x, int n_param_in, double min_prob, double* unpaired, const MeaOut* mea) {
  stream_listed(&Engine::pairs_, n_param_in, [&](int c0, size_t at, Engine& e) {
    int64_t m = 0;
    MeaOut mc;
    if (mea) mc = MeaOut{mea->gamma, mea->structure ? mea->structure + at : nullptr, mea->score ? mea->score + c0 : nullptr};
    e.pair_posteriors(x, n_param_in, min_prob, &m, unpaired ? unpaired + at : nullptr, mea ? &mc : nullptr);
  });
}

void Engine::pair_list(int32_t* seq, int32_t* i, int32_t* j, double* p, int64_t cap) {
  require_device();
  DeviceGuard dg(device_);
  pairs_.fetch(seq, i, j, p, nullptr, nullptr, cap);
}


// ---- motif-conditional pair posteriors (cond_rules.h).  Per group, queued on its stream behind one another on its
// table slots: the inside sweep (SCAN_PASS_INSIDE, with the train evaluation's range check over all three Z), the outside sweep
// seeded with the ari terminals and the reduction of the P plane with Z(ari), the outside sweep seeded with the nasi terminal
// into the same outside slot and the reduction with Z(nasi), the per-sequence pass over both worlds, the two MEA decodes.  The
// log-space form -- the fused scan kernel up to its inside pass, then one outside pass and one reduction per world -- for the
// sequences that leave the double range and under pipeline 3.  Then the batch list in (sequence, i, j) order with two probability
// columns, in buffers of its own: the list of the last pair call is left alone.
void Engine::pair_conditional(const double* x, int n_param_in, double min_prob, int64_t* n_pairs, const CondOut& out) {
  require_device();
  DeviceGuard dg(device_);
  if (!n_pairs) throw ArgError("pair_conditional: null n_pairs");
  if (!(min_prob >= 0.)) throw ArgError("pair_conditional: min_prob must be >= 0");
  const bool mea = out.structure[0] || out.structure[1];
  if (mea && !(std::isfinite(out.gamma) && out.gamma > 0.)) throw ArgError("pair_conditional: gamma must be finite and > 0");
  if (streaming_) { stream_cond(x, n_param_in, min_prob, out); *n_pairs = conds_.count(); return; }
  require_resident("pair_conditional", n_param_in);
  conds_.invalidate();
  upload_params(x, lay_, false);
  const int n = n_seq_;
  const size_t n_seqpos = (size_t)h_seq_off_[n];
  const size_t pcells = (size_t)(Lmax_ + 1) * (Wmax_ + 1);   // P(i, d) of one world of one table slot
  ScanPos pos(n_seqpos, n);
  d_cd_unp_[0].alloc(8 * n_seqpos); d_cd_unp_[1].alloc(8 * n_seqpos);
  d_cd_exist_.alloc(8 * (size_t)n); d_cd_shift_.alloc(8 * (size_t)n);
  HIP_OK(hipEventRecord(ev_[1], st_));
  const StagedList::Staging sl = conds_.begin(plan_.d_plans.as<SeqPlan>(), d_okbits1_.as<uint32_t>(), n, 1, st_);
  CondArgs ca;
  std::memset(&ca, 0, sizeof(ca));
  ca.plans = plan_.d_plans.as<SeqPlan>();
  ca.okbits = d_okbits1_.as<uint32_t>();
  ca.seq_out = d_seq_out_.as<double>(); ca.out_stride = out_stride_;
  ca.p_stride = pcells;
  ca.min_prob = min_prob;
  ca.unpaired[0] = d_cd_unp_[0].as<double>(); ca.unpaired[1] = d_cd_unp_[1].as<double>();
  ca.exist = d_cd_exist_.as<double>(); ca.shift = d_cd_shift_.as<double>();
  ca.koff = sl.koff; ca.cnt = sl.cnt;
  ca.st_i = sl.st_i; ca.st_j = sl.st_j;
  ca.st_p[0] = sl.st_v[0]; ca.st_p[1] = sl.st_v[1];
  // the scratch per slot: P of either world; MEA: the M table and the choices, which the two decodes of a slot share
  const size_t mea_ch_stride = pcells + (size_t)Lmax_ + 1;
  auto at_slot = [&](CondArgs& ck, PairArgs& pk, size_t slot0) {
    for (int w = 0; w < 2; ++w) ck.P[w] = slot_scratch<double>(d_cd_P_[w], pcells, slot0);
    if (!mea) return;
    pk.mea_M = slot_scratch<double>(d_cd_M_, pcells, slot0);
    pk.mea_ch = slot_scratch<int32_t>(d_cd_ch_, mea_ch_stride, slot0);
  };
  // the MEA decode of both worlds: the pair call's kernel over the world's P and unpaired (the scores are not handed out)
  PairArgs pm = pair_batch_args();
  pm.p_stride = pcells;
  if (mea) {
    d_cd_s_[0].alloc(n_seqpos); d_cd_s_[1].alloc(n_seqpos); d_cd_sc_.alloc(8 * 2 * (size_t)n);
    pm.mea_gamma2 = 2. * out.gamma;
    pm.mea_ch_stride = mea_ch_stride;
  }
  auto launch_mea = [&](const CondArgs& ck, PairArgs pk, int G, hipStream_t st) {
    if (!mea) return;
    for (int w = 0; w < 2; ++w) {
      if (!out.structure[w]) continue;
      pk.idx = ck.idx;
      pk.skip_flagged = ck.skip_flagged;
      pk.P = ck.P[w];
      pk.unpaired = ck.unpaired[w];
      pk.mea_s = d_cd_s_[w].as<char>(); pk.mea_score = d_cd_sc_.as<double>() + (size_t)w * n;
      HIP_OK(launch_pair_mea(pk, G, Wmax_, st));
    }
  };
  const int n_flagged = scan_both_forms(pos, [&](LinArgs& a) {
    at_slot(ca, pm, 0);
    a.range_all = 1;
    PairArgs pp = pair_batch_args();
    pair_plane_fields(pp, a);
    ca.p_cs = pp.p_cs; ca.p_rs = pp.p_rs; ca.ncol = pp.ncol; ca.band_stride = pp.band_stride;
    ca.skip_flagged = 1;
  }, [&](const LinArgs& ak, size_t slot0, int G, int Lg, int Wg, hipStream_t st) {
    CondArgs ck = ca;
    PairArgs pk = pm;
    ck.idx = ak.grp;
    ck.band_in = ak.band_in; ck.band_out = ak.band_out; ck.z = ak.zs; ck.z_log = 0;
    at_slot(ck, pk, slot0);
    const int cells = (Lg + 1) * (Wg + 1);
    HIP_OK(launch_lin_scan_group(ak, G, Lg, Wg, SCAN_PASS_INSIDE, st));
    HIP_OK(launch_lin_scan_group(ak, G, Lg, Wg, SCAN_PASS_OUT_ARI, st));
    HIP_OK(launch_cond_cells(ck, COND_MOTIF, G, cells, st));
    HIP_OK(launch_lin_scan_group(ak, G, Lg, Wg, SCAN_PASS_OUT_NASI, st));   // (into the same outside slot)
    HIP_OK(launch_cond_cells(ck, COND_NONE, G, cells, st));
    HIP_OK(launch_cond_seq(ck, G, st));
    launch_mea(ck, pk, G, st);
  },
  // ---- the log-space form, in chunks of at most as many sequences as the scratch holds
  [&](DpArgs& d, int n_blocks, int n_log) {
    const int chunk = log_chunk(n_blocks, n_log);
    at_slot(ca, pm, 0);
    d_cd_z_.alloc(8 * 4 * (size_t)chunk);
    d.cond_p0 = ca.P[0];
    d.cond_p1 = ca.P[1];
    d.cond_z = d_cd_z_.as<double>();
    d.pair_stride = pcells;
    return chunk;
  }, [&](const int32_t* idx, int C) {
    CondArgs ck = ca;
    ck.idx = idx;
    ck.skip_flagged = 0;
    ck.z = d_cd_z_.as<double>(); ck.z_log = 1;
    HIP_OK(launch_cond_seq(ck, C, st_));
    launch_mea(ck, pm, C, st_);
  }, false);   // (both worlds by definition: option world does not apply)
  finish_call(n_flagged, [&] { *n_pairs = conds_.finish(st_); });   // the list in (sequence, i, j) order
  auto get = [&](void* dst, const DevBuf& src, size_t bytes) { if (dst && bytes) HIP_OK(hipMemcpy(dst, src.as<void>(), bytes, hipMemcpyDeviceToHost)); };
  get(out.exist, d_cd_exist_, 8 * (size_t)n);
  get(out.shift, d_cd_shift_, 8 * (size_t)n);
  for (int w = 0; w < 2; ++w) {
    get(out.unpaired[w], d_cd_unp_[w], 8 * n_seqpos);
    if (mea) get(out.structure[w], d_cd_s_[w], n_seqpos);
  }
}

void Engine::stream_cond(const double* x, int n_param_in, double min_prob, const CondOut& out) {
  conds_.invalidate();
  stream_listed(&Engine::conds_, n_param_in, [&](int c0, size_t at, Engine& e) {
    int64_t m = 0;
    CondOut oc{out.gamma, out.exist ? out.exist + c0 : nullptr,
               {out.unpaired[0] ? out.unpaired[0] + at : nullptr, out.unpaired[1] ? out.unpaired[1] + at : nullptr},
               {out.structure[0] ? out.structure[0] + at : nullptr, out.structure[1] ? out.structure[1] + at : nullptr},
               out.shift ? out.shift + c0 : nullptr};
    e.pair_conditional(x, n_param_in, min_prob, &m, oc);
  });
}

void Engine::cond_list(int32_t* seq, int32_t* i, int32_t* j, double* p_motif, double* p_none, int64_t cap) {
  require_device();
  DeviceGuard dg(device_);
  conds_.fetch(seq, i, j, p_motif, p_none, nullptr, cap);
}


// ---- structural context profiles under the motif model (ctx_rules.h).  The scan's first sum pass per group, then
// on the group's table slots, before the next group of the stream reuses them: the pair reduction (k4_pairs), the per-run values
// and the exterior column (k_ctx_cells), the seven columns per position (k_ctx_seq).  The log-space form -- the fused scan kernel
// up to its first outside pass, then the same rule on its dense tables -- for the sequences that leave the double range and under
// pipeline 3, with k_ctx_seq behind every launch.  Leaves the list of the last pair call alone.
void Engine::context_profile(const double* x, int n_param_in, double* profile) {
  require_device();
  DeviceGuard dg(device_);
  if (!profile) throw ArgError("context_profile: null profile");
  if (streaming_) {
    stream_call(n_param_in, [] {}, [&](int c0, int, Engine& e) {
      e.context_profile(x, n_param_in, profile + (size_t)kCtxCols * (size_t)(h_seq_off_[c0] - h_seq_off_[0]));
    });
    return;
  }
  require_resident("context_profile", n_param_in);
  upload_params(x, lay_, false);
  const int n = n_seq_;
  const size_t n_seqpos = (size_t)h_seq_off_[n];
  const size_t pcells = (size_t)(Lmax_ + 1) * (Wmax_ + 1);   // one [i][d] array of a table slot
  const size_t ocol = (size_t)Lmax_ + 1;
  ScanPos pos(n_seqpos, n);
  d_cx_prof_.alloc(8 * kCtxCols * std::max<size_t>(n_seqpos, 1));
  HIP_OK(hipEventRecord(ev_[1], st_));
  CtxArgs ca;
  std::memset(&ca, 0, sizeof(ca));
  ca.plans = plan_.d_plans.as<SeqPlan>();
  ca.seq_out = d_seq_out_.as<double>(); ca.out_stride = out_stride_;
  ca.c_stride = 4 * pcells;
  ca.o_stride = ocol;
  ca.profile = d_cx_prof_.as<double>();
  ca.no_rss = (flags_ & ELEMDP_NO_RSS) ? 1 : 0;
  auto at_slot = [&](CtxArgs& ck, size_t slot0) {
    ck.P = slot_scratch<double>(d_cx_cells_, 4 * pcells, slot0);
    ck.u = ck.P + pcells; ck.h = ck.P + 2 * pcells; ck.b = ck.P + 3 * pcells;
    ck.o = slot_scratch<double>(d_cx_o_, ocol, slot0);
  };
  PairArgs pa = pair_batch_args();
  pa.p_stride = 4 * pcells;
  const int n_flagged = scan_both_forms(pos, [&](LinArgs& a) {
    at_slot(ca, 0);
    pair_plane_fields(pa, a);
    ca.skip_flagged = 1;
  }, [&](const LinArgs& ak, size_t slot0, int G, int Lg, int Wg, hipStream_t st) {
    HIP_OK(launch_lin_world_group(ak, G, Lg, Wg, st));
    CtxArgs ck = ca;
    ck.idx = ak.grp;
    at_slot(ck, slot0);
    if (!ca.no_rss) {
      PairArgs pk = pa;
      pk.idx = ak.grp;
      pk.band_in = ak.band_in; pk.band_out = ak.band_out; pk.zs = ak.zs + ak.world;
      pk.P = ck.P;
      HIP_OK(launch_pair_cells(pk, G, (Lg + 1) * (Wg + 1), st));
      HIP_OK(launch_ctx_cells(ak, ck, G, (Lg + 1) * (Wg + 1), st));
    }
    HIP_OK(launch_ctx_seq(ck, G, st));
  },
  // ---- the log-space form, in chunks of at most as many sequences as the scratch holds
  [&](DpArgs& d, int n_blocks, int n_log) {
    at_slot(ca, 0);
    d.ctx = ca;
    return log_chunk(n_blocks, n_log);
  }, [&](const int32_t* idx, int C) {
    CtxArgs ck = ca;
    ck.idx = idx;
    ck.skip_flagged = 0;
    HIP_OK(launch_ctx_seq(ck, C, st_));
  });
  // (the whole call includes the profile's way to the host: 7 doubles per position, 112 MB for 10 000 sequences of L = 200)
  finish_call(n_flagged, [&] {
    if (n_seqpos) HIP_OK(hipMemcpyAsync(profile, d_cx_prof_.as<void>(), 8 * kCtxCols * n_seqpos, hipMemcpyDeviceToHost, st_));
  });
}


// ---- accessibility under the motif model (access_rules.h).  The scan's first sum pass per group, then on the
// group's table slots, before the next group of the stream reuses them: the chains of the four terms (k_access_chains) and the
// windows of every position (k_access_seq).  The log-space form -- the fused scan kernel up to its first outside pass, then the
// same rule on its dense tables -- for the sequences that leave the double range and under pipeline 3, with k_access_seq behind
// every launch.  Every buffer is the call's own: leaves the list of the last pair call alone.
void Engine::accessibility(const double* x, int n_param_in, int max_width, double* access) {
  require_device();
  DeviceGuard dg(device_);
  if (!access) throw ArgError("accessibility: null access");
  if (max_width < 1 || max_width > kAccessMaxWidth) throw ArgError("accessibility: max_width must lie in 1 .. 64");
  const int U = max_width;
  if (streaming_) {
    stream_call(n_param_in, [] {}, [&](int c0, int, Engine& e) {
      e.accessibility(x, n_param_in, U, access + (size_t)U * (size_t)(h_seq_off_[c0] - h_seq_off_[0]));
    });
    return;
  }
  require_resident("accessibility", n_param_in);
  upload_params(x, lay_, false);
  const int n = n_seq_;
  const size_t n_seqpos = (size_t)h_seq_off_[n];
  const size_t plane = ((size_t)Lmax_ + 1) * U;   // one term of a slot: U sums per position 0 .. L
  ScanPos pos(n_seqpos, n);
  d_ac_out_.alloc(8 * (size_t)U * std::max<size_t>(n_seqpos, 1));
  HIP_OK(hipEventRecord(ev_[1], st_));
  AccessArgs ca;
  std::memset(&ca, 0, sizeof(ca));
  ca.plans = plan_.d_plans.as<SeqPlan>();
  ca.seq_out = d_seq_out_.as<double>(); ca.out_stride = out_stride_;
  ca.U = U;
  ca.terms = opt_access_terms_;
  ca.plane = plane; ca.t_stride = ACC_TERMS * plane;
  ca.access = d_ac_out_.as<double>();
  ca.no_rss = (flags_ & ELEMDP_NO_RSS) ? 1 : 0;
  auto at_slot = [&](AccessArgs& ck, size_t slot0) { ck.T = slot_scratch<double>(d_ac_T_, ACC_TERMS * plane, slot0); };
  int n_vec = 0;
  const int n_flagged = scan_both_forms(pos, [&](LinArgs& a) {
    at_slot(ca, 0);
    n_vec = std::max(a.lay.S, a.lay.n_ap);   // (entries of a state vector: the interval states, the pairs of rule 2)
    ca.skip_flagged = 1;
  }, [&](const LinArgs& ak, size_t slot0, int G, int Lg, int Wg, hipStream_t st) {
    HIP_OK(launch_lin_world_group(ak, G, Lg, Wg, st));
    AccessArgs ck = ca;
    ck.idx = ak.grp;
    at_slot(ck, slot0);
    if (!ca.no_rss) HIP_OK(launch_access_chains(ak, ck, G, Lg, n_vec, st));
    HIP_OK(launch_access_seq(ck, G, st));
  },
  // ---- the log-space form, in chunks of at most as many sequences as the scratch holds
  [&](DpArgs& d, int n_blocks, int n_log) {
    at_slot(ca, 0);
    // (a launch has at most n_blocks workgroups, each with 64 lanes on units: 2 S doubles per lane, 22 KB per workgroup at S = 22)
    d_ac_vec_.alloc(8 * 2 * (size_t)d.lay.S * 64 * (size_t)std::max(n_blocks, 1));
    d.acc = ca;
    d.acc.vec = d_ac_vec_.as<double>();
    return log_chunk(n_blocks, n_log);
  }, [&](const int32_t* idx, int C) {
    AccessArgs ck = ca;
    ck.idx = idx;
    ck.skip_flagged = 0;
    HIP_OK(launch_access_seq(ck, C, st_));
  });
  finish_call(n_flagged, [&] {
    if (n_seqpos) HIP_OK(hipMemcpyAsync(access, d_ac_out_.as<void>(), 8 * (size_t)U * n_seqpos, hipMemcpyDeviceToHost, st_));
  });
}


// ---- posterior motif-node profiles under the motif model (node_rules.h).  The scan's first sum pass per group,
// then k_node_pos on the group's table slots, before the next group of the stream reuses them; the log-space form -- the fused
// scan kernel up to its first outside pass, then the same rule on its dense tables -- for the sequences that leave the double
// range and under pipeline 3.  Both forms write the profile of the call directly: no scratch per slot.  Leaves the list of the
// last pair call alone.
void Engine::node_profile(const double* x, int n_param_in, double* profile) {
  require_device();
  DeviceGuard dg(device_);
  if (!profile) throw ArgError("node_profile: null profile");
  const int M = au_.M();
  if (M > 255) throw ArgError("node_profile: more than 255 pattern nodes");
  if (streaming_) {
    stream_call(n_param_in, [] {}, [&](int c0, int, Engine& e) {
      e.node_profile(x, n_param_in, profile + (size_t)M * (size_t)(h_seq_off_[c0] - h_seq_off_[0]));
    });
    return;
  }
  const int n_flagged = node_profile_device("node_profile", x, n_param_in);
  const size_t n_seqpos = (size_t)h_seq_off_[n_seq_];
  finish_call(n_flagged, [&] {
    if (n_seqpos) HIP_OK(hipMemcpyAsync(profile, d_nd_prof_.as<void>(), 8 * (size_t)M * n_seqpos, hipMemcpyDeviceToHost, st_));
  });
}

// The profile of the resident batch on the device (d_nd_prof_), both forms, queued on the engine's stream behind ev_[1]; returns
// the number of sequences handed to the log-space form.  The step node_profile and node_mea share.
int Engine::node_profile_device(const char* what, const double* x, int n_param_in) {
  const int M = au_.M();
  require_resident(what, n_param_in);
  upload_params(x, lay_, false);
  const int n = n_seq_;
  const size_t n_seqpos = (size_t)h_seq_off_[n];
  ScanPos pos(n_seqpos, n);
  d_nd_prof_.alloc(8 * (size_t)M * std::max<size_t>(n_seqpos, 1));
  std::vector<int32_t> lists;
  node_lists_build(lay_, ints_.data(), &lists);
  d_nd_lists_.upload(lists, st_);
  HIP_OK(hipStreamSynchronize(st_));   // (the host vector goes out of use with the copy)
  HIP_OK(hipEventRecord(ev_[1], st_));
  NodeArgs na;
  std::memset(&na, 0, sizeof(na));
  na.lists = d_nd_lists_.as<int32_t>();
  na.M = M;
  na.rules = opt_node_rules_;
  na.no_rss = (flags_ & ELEMDP_NO_RSS) ? 1 : 0;
  na.profile = d_nd_prof_.as<double>();
  return scan_both_forms(pos, [&](LinArgs& a) {
    if (a.lay.shadow >= 0 || a.lay.S != lay_.S) throw std::logic_error("node_profile: the scan sweeps another automaton than the lists name");
  }, [&](const LinArgs& ak, size_t, int G, int Lg, int Wg, hipStream_t st) {
    HIP_OK(launch_lin_world_group(ak, G, Lg, Wg, st));
    HIP_OK(launch_node_pos(ak, na, G, Lg, st));
  }, [&](DpArgs& d, int, int n_log) {
    d.node = na;
    return std::max(n_log, 1);
  }, [&](const int32_t*, int) {});
}


// ---- joint node-by-context posteriors and emission counts (joint_rules.h).  The scan's first sum pass per group,
// then on the group's table slots, before the next group of the stream reuses them: the hairpin and bulge chains of every row
// (k_joint_rows), the 7 M columns of every position (k_joint_pos), the counts (k_joint_counts).  The log-space form -- the fused
// scan kernel up to its first outside pass, then the same rule on its dense tables -- for the sequences that leave the double range
// and under pipeline 3, with k_joint_counts behind the launch.  The profile goes to the host only where the caller gave a buffer.
// Every buffer is the call's own: leaves the list of the last pair call alone.
void Engine::joint_profile(const double* x, int n_param_in, double* counts, double* profile) {
  require_device();
  DeviceGuard dg(device_);
  if (!counts) throw ArgError("joint_profile: null counts");
  const int M = au_.M();
  if (M > 255) throw ArgError("joint_profile: more than 255 pattern nodes");
  const size_t row = (size_t)kCtxCols * M, nc = row * kJointBases;
  if (streaming_) {
    stream_call(n_param_in, [] {}, [&](int c0, int, Engine& e) {
      e.joint_profile(x, n_param_in, counts + nc * (size_t)c0, profile ? profile + row * (size_t)(h_seq_off_[c0] - h_seq_off_[0]) : nullptr);
    });
    return;
  }
  require_resident("joint_profile", n_param_in);
  upload_params(x, lay_, false);
  const int n = n_seq_;
  const size_t n_seqpos = (size_t)h_seq_off_[n];
  ScanPos pos(n_seqpos, n);
  d_jn_prof_.alloc(8 * row * std::max<size_t>(n_seqpos, 1));
  d_jn_counts_.alloc(8 * nc * (size_t)n);
  std::vector<int32_t> lists;
  size_t slot_at = 0;
  const int n_slots = joint_lists_build(lay_, ints_.data(), &lists, &slot_at);
  d_jn_lists_.upload(lists, st_);
  HIP_OK(hipStreamSynchronize(st_));   // (the host vector goes out of use with the copy)
  HIP_OK(hipEventRecord(ev_[1], st_));
  JointArgs ja;
  std::memset(&ja, 0, sizeof(ja));
  ja.plans = plan_.d_plans.as<SeqPlan>();
  ja.seq_out = d_seq_out_.as<double>(); ja.out_stride = out_stride_;
  ja.seq = d_seq_.as<uint8_t>();
  ja.lists = d_jn_lists_.as<int32_t>();
  ja.slot_at = (int32_t)slot_at; ja.n_slots = n_slots;
  ja.M = M;
  ja.no_rss = (flags_ & ELEMDP_NO_RSS) ? 1 : 0;
  ja.x_stride = joint_scratch_size(Lmax_, Wmax_, n_slots);
  ja.profile = d_jn_prof_.as<double>();
  ja.counts = d_jn_counts_.as<double>();
  const int n_flagged = scan_both_forms(pos, [&](LinArgs& a) {
    if (a.lay.shadow >= 0 || a.lay.S != lay_.S) throw std::logic_error("joint_profile: the scan sweeps another automaton than the lists name");
    ja.X = slot_scratch<double>(d_jn_X_, ja.x_stride);
    ja.skip_flagged = 1;
  }, [&](const LinArgs& ak, size_t slot0, int G, int Lg, int Wg, hipStream_t st) {
    HIP_OK(launch_lin_world_group(ak, G, Lg, Wg, st));
    JointArgs jk = ja;
    jk.idx = ak.grp;
    jk.X = slot_scratch<double>(d_jn_X_, ja.x_stride, slot0);
    if (!ja.no_rss) HIP_OK(launch_joint_rows(ak, jk, G, Lg, st));
    HIP_OK(launch_joint_pos(ak, jk, G, Lg, st));
    HIP_OK(launch_joint_counts(jk, G, st));
  },
  // ---- the log-space form: one launch, the scratch and the vectors per workgroup (not per sequence: what the sum passes left
  // serves where it is large enough)
  [&](DpArgs& d, int n_blocks, int n_log) {
    const size_t nb = (size_t)std::max(n_blocks, 1);
    if (opt_pipeline_ != 4 || d_jn_X_.bytes() < 8 * ja.x_stride * nb) d_jn_X_.alloc(8 * ja.x_stride * nb);
    d_jn_vec_.alloc(8 * 5 * (size_t)d.lay.S * kThreads * nb);
    d.jnt = ja;
    d.jnt.X = d_jn_X_.as<double>();
    d.jnt.vec = d_jn_vec_.as<double>();
    return std::max(n_log, 1);
  }, [&](const int32_t* idx, int C) {
    JointArgs jk = ja;
    jk.idx = idx;
    jk.skip_flagged = 0;
    HIP_OK(launch_joint_counts(jk, C, st_));
  });
  finish_call(n_flagged, [&] {
    HIP_OK(hipMemcpyAsync(counts, d_jn_counts_.as<void>(), 8 * nc * (size_t)n, hipMemcpyDeviceToHost, st_));
    if (profile && n_seqpos) HIP_OK(hipMemcpyAsync(profile, d_jn_prof_.as<void>(), 8 * row * n_seqpos, hipMemcpyDeviceToHost, st_));
  });
}

// ---- the stem slots of the automaton (stem_rules.h): host only, no device needed
int Engine::stem_slots(int32_t* node_left, int32_t* node_right, int cap) const {
  std::vector<int32_t> lists;
  const int K = stem_lists_build(lay_, ints_.data(), &lists);
  if (!node_left && !node_right) return K;
  if (cap < K) throw ArgError("stem_slots: buffer too small");
  for (int k = 0; k < K; ++k) {   // (the node pairs behind the K + 1 offsets: StemLists::left / right)
    if (node_left) node_left[k] = lists[K + 1 + 2 * k];
    if (node_right) node_right[k] = lists[K + 2 + 2 * k];
  }
  return K;
}

// ---- pair posteriors by motif node pair and the pair counts behind a stem logo (stem_rules.h).  The scan's first
// sum pass per group, then on the group's table slots, before the next group of the stream reuses them: Q of every cell by stem
// slot (k_stem_cells), the counts (k_stem_counts) and, with a finite min_prob, the list entries into the staging ranges
// (k_stem_seq).  The log-space form -- the fused scan kernel up to its first outside pass, then the same rule on its dense tables
// -- for the sequences that leave the double range and under pipeline 3, with the same two kernels behind the launch.  Then the
// batch list in (sequence, i, j, slot) order.  The staging is sized by the bound kept cells x K.  Every buffer is the call's own:
// leaves the lists of the last pair call and the last conditional call alone.
void Engine::stem_profile(const double* x, int n_param_in, double min_prob, double* counts, int64_t* n_entries) {
  require_device();
  DeviceGuard dg(device_);
  if (!counts) throw ArgError("stem_profile: null counts");
  if (!(min_prob >= 0.)) throw ArgError("stem_profile: min_prob must be >= 0");
  std::vector<int32_t> lists;
  const int K = stem_lists_build(lay_, ints_.data(), &lists);
  if (K > kStemMaxSlots || au_.M() > 255) throw ArgError("stem_profile: more than 255 stem slots or pattern nodes");
  const size_t nc = (size_t)K * kStemBlock;
  const bool want_list = min_prob < HUGE_VAL;
  stems_.invalidate();
  if (streaming_) {
    stream_listed(&Engine::stems_, n_param_in, [&](int c0, size_t, Engine& e) { e.stem_profile(x, n_param_in, min_prob, counts + nc * (size_t)c0, nullptr); });
    if (n_entries) *n_entries = stems_.count();
    return;
  }
  require_resident("stem_profile", n_param_in);
  upload_params(x, lay_, false);
  const int n = n_seq_;
  const size_t n_seqpos = (size_t)h_seq_off_[n];
  ScanPos pos(n_seqpos, n);
  d_sp_counts_.alloc(8 * std::max<size_t>(nc, 1) * (size_t)n);
  d_sp_has_.alloc(4 * (size_t)n);
  d_sp_lists_.upload(lists, st_);
  HIP_OK(hipMemsetAsync(d_sp_has_.as<void>(), 0, 4 * (size_t)n, st_));
  HIP_OK(hipStreamSynchronize(st_));   // (the host vector goes out of use with the copy; the marks are clear before any group runs)
  HIP_OK(hipEventRecord(ev_[1], st_));
  StemArgs sa;
  std::memset(&sa, 0, sizeof(sa));
  sa.plans = plan_.d_plans.as<SeqPlan>();
  sa.seq_out = d_seq_out_.as<double>(); sa.out_stride = out_stride_;
  sa.seq = d_seq_.as<uint8_t>();
  sa.okbits = d_okbits1_.as<uint32_t>();
  sa.lists = d_sp_lists_.as<int32_t>();
  sa.K = K; sa.n_list = (int32_t)lists.size();
  sa.x_stride = stem_scratch_size(Lmax_, Wmax_, K);
  sa.has = d_sp_has_.as<int32_t>();
  sa.counts = d_sp_counts_.as<double>();
  sa.min_prob = min_prob;
  if (want_list) {   // staging ranges: a sequence's list holds at most K entries per kept cell
    const StagedList::Staging sl = stems_.begin(plan_.d_plans.as<SeqPlan>(), d_okbits1_.as<uint32_t>(), n, K, st_);
    sa.koff = sl.koff; sa.cnt = sl.cnt;
    sa.st_i = sl.st_i; sa.st_j = sl.st_j; sa.st_k = sl.st_k; sa.st_q = sl.st_v[0];
  }
  const bool no_rss = (flags_ & ELEMDP_NO_RSS) != 0;
  const int n_flagged = scan_both_forms(pos, [&](LinArgs& a) {
    if (a.lay.shadow >= 0 || a.lay.S != lay_.S) throw std::logic_error("stem_profile: the scan sweeps another automaton than the lists name");
    sa.X = slot_scratch<double>(d_sp_X_, sa.x_stride);
    sa.skip_flagged = 1;
  }, [&](const LinArgs& ak, size_t slot0, int G, int Lg, int Wg, hipStream_t st) {
    HIP_OK(launch_lin_world_group(ak, G, Lg, Wg, st));
    StemArgs sk = sa;
    sk.idx = ak.grp;
    sk.X = slot_scratch<double>(d_sp_X_, sa.x_stride, slot0);
    if (!no_rss) HIP_OK(launch_stem_cells(ak, sk, G, (Lg + 1) * (Wg + 1), st));   // (else no mark is set: the band tables are not read)
    HIP_OK(launch_stem_counts(sk, G, Lg, Wg, st));
    if (want_list) HIP_OK(launch_stem_seq(sk, G, st));
  },
  // ---- the log-space form, in chunks of at most as many sequences as the table slots hold (the scratch is bounded by the chunk)
  [&](DpArgs& d, int n_blocks, int n_log) {
    sa.X = slot_scratch<double>(d_sp_X_, sa.x_stride);
    d.stm = sa;
    return log_chunk(n_blocks, n_log);
  }, [&](const int32_t* idx, int C) {
    StemArgs sk = sa;
    sk.idx = idx;
    sk.skip_flagged = 0;
    HIP_OK(launch_stem_counts(sk, C, Lmax_, Wmax_, st_));
    if (want_list) HIP_OK(launch_stem_seq(sk, C, st_));
  });
  finish_call(n_flagged, [&] {
    if (want_list) stems_.finish(st_); else stems_.set_empty();   // the list in (sequence, i, j, slot) order
    if (nc) HIP_OK(hipMemcpyAsync(counts, d_sp_counts_.as<void>(), 8 * nc * (size_t)n, hipMemcpyDeviceToHost, st_));
  });
  if (n_entries) *n_entries = stems_.count();
}

void Engine::stem_list(int32_t* seq, int32_t* i, int32_t* j, int32_t* slot, double* q, int64_t cap) {
  require_device();
  DeviceGuard dg(device_);
  stems_.fetch(seq, i, j, q, nullptr, slot, cap);
}

// ---- the items -- stems or loops -- of the structures a caller hands to helix_posteriors or loop_posteriors (structure_rules.h):
// per sequence the range off[t] .. off[t + 1] of items, of an item its 5' position i, a label (the stem's length, the loop's type)
// and, behind the call, its probability p.  The further columns of an item are the call's own.
static_assert(LOOP_H == 1 && LOOP_S == 2 && LOOP_B == 3 && LOOP_I == 4 && LOOP_M == 5, "structure_loops writes the types as numbers");
struct StructItems {
  std::vector<int64_t> off; std::vector<int32_t> i, label; std::vector<double> p;
  // One sequence after the other: the mates of its structure, or the refusal "<call>: what is wrong"; add(mate, L) appends its items.
  template <class Add> void parse(const char* call, const char* structure, const std::vector<int32_t>& seq_off, int n, Add add) {
    off.assign((size_t)n + 1, 0);
    std::vector<int32_t> mate;
    for (int t = 0; t < n; ++t) {
      const int L = seq_off[t + 1] - seq_off[t];
      mate.resize((size_t)L);
      const char* err = structure_mates(structure + (seq_off[t] - seq_off[0]), L, mate.data());
      if (*err) throw ArgError(std::string(call) + ": " + err);
      add(mate.data(), L);
      off[(size_t)t + 1] = (int64_t)i.size();
    }
    p.assign(i.size(), 0.);
  }
  // Offsets, then the columns given, to the device on st; clears p there; waits (the host vectors go out of use, p is clear before any group runs).
  using Col = std::pair<DevBuf*, const std::vector<int32_t>*>;
  void upload_cleared(DevBuf& d_off, std::initializer_list<Col> cols, DevBuf& d_p, hipStream_t st) const {
    d_off.upload(off, st);
    for (const Col& c : cols) c.first->upload(*c.second, st);
    d_p.alloc(8 * std::max<size_t>(p.size(), 1));
    HIP_OK(hipMemsetAsync(d_p.as<void>(), 0, 8 * std::max<size_t>(p.size(), 1), st));
    HIP_OK(hipStreamSynchronize(st));
  }
  void download(const DevBuf& d_p, hipStream_t st) {   // (queued: p holds the probabilities once st has been waited for)
    if (!p.empty()) HIP_OK(hipMemcpyAsync(p.data(), d_p.as<void>(), 8 * p.size(), hipMemcpyDeviceToHost, st));
  }
  // The caller's columns per position (either may be null): label and p at the position of every item, 0 and NaN elsewhere.
  void write(const std::vector<int32_t>& seq_off, int n, int32_t* label_out, double* prob_out) const {
    const size_t n_seqpos = (size_t)(seq_off[n] - seq_off[0]);
    if (label_out) std::fill(label_out, label_out + n_seqpos, 0);
    if (prob_out) std::fill(prob_out, prob_out + n_seqpos, std::nan(""));
    for (int t = 0; t < n; ++t)
      for (int64_t k = off[t]; k < off[(size_t)t + 1]; ++k) {
        const size_t at = (size_t)(seq_off[t] - seq_off[0]) + (size_t)i[(size_t)k];
        if (label_out) label_out[at] = label[(size_t)k];
        if (prob_out) prob_out[at] = p[(size_t)k];
      }
  }
};

// The loop call's launch_helix_units: the compaction of the helix call, the kept cells whose P reaches helix_pick_bound(min_prob) = the bound
static HelixArgs loop_unit_pick(const LoopArgs& lk, double min_prob) {
  HelixArgs hk;
  std::memset(&hk, 0, sizeof(hk));
  hk.plans = lk.plans; hk.idx = lk.idx; hk.seq_out = lk.seq_out; hk.out_stride = lk.out_stride; hk.skip_flagged = 1;
  hk.okbits = lk.okbits; hk.min_prob = min_prob; hk.P = lk.P; hk.p_stride = lk.p_stride;
  hk.n_units = lk.n_units; hk.ui = lk.ui; hk.ud = lk.ud; hk.u_stride = lk.u_stride;
  return hk;
}

// ---- helix posteriors (helix_rules.h).  The host parses the stems of the caller's structures.  The scan's first sum
// pass per group, then on the group's table slots, before the next group of the stream reuses them: P of every cell (k4_pairs), the
// units -- the kept cells whose P reaches min_prob -- (k_helix_units), the chains of the units and of the stems (k_helix_chains) and
// the list entries into the staging ranges (k_helix_seq).  The log-space form -- the fused scan kernel up to its first outside pass,
// then the same chain on its dense tables -- for the sequences that leave the double range and under pipeline 3, with k_helix_seq
// behind the launch.  Then the batch list in (sequence, i, j, len) order.  The staging is sized by the bound kept cells x
// (max_len - min_len + 1).  Every buffer is the call's own: leaves the lists of the last pair, conditional and stem call alone.
void Engine::helix_posteriors(const double* x, int n_param_in, int max_len, int min_len, double min_prob, int64_t* n_entries,
                              const char* structure, int32_t* stem_len, double* stem_prob) {
  require_device();
  DeviceGuard dg(device_);
  if (max_len < 1 || max_len > kHelixMaxLen) throw ArgError("helix_posteriors: max_len must lie in 1 .. 32");
  if (min_len < 1 || min_len > max_len) throw ArgError("helix_posteriors: min_len must lie in 1 .. max_len");
  if (!(min_prob >= 0.)) throw ArgError("helix_posteriors: min_prob must be >= 0");
  if (structure && !stem_len && !stem_prob) throw ArgError("helix_posteriors: a structure needs stem_len or stem_prob");
  if (n_seq_ <= 0) throw StateError("helix_posteriors before load_batch");
  const int n = n_seq_;
  const bool want_list = min_prob < HUGE_VAL;
  // the stems of every sequence: (i, d, len) of the outermost pair, sequences and 5' ends in increasing order; the label is len
  StructItems stems;
  std::vector<int32_t> s_d;
  if (structure)
    stems.parse("helix_posteriors", structure, h_seq_off_, n, [&](const int32_t* mate, int L) { structure_stems(mate, L, &stems.i, &s_d, &stems.label); });
  helices_.invalidate();
  if (streaming_) {
    stream_listed(&Engine::helices_, n_param_in, [&](int, size_t at, Engine& e) {
      e.helix_posteriors(x, n_param_in, max_len, min_len, min_prob, nullptr, structure ? structure + at : nullptr,
                         stem_len ? stem_len + at : nullptr, stem_prob ? stem_prob + at : nullptr);
    });
    if (n_entries) *n_entries = helices_.count();
    return;
  }
  require_resident("helix_posteriors", n_param_in);
  upload_params(x, lay_, false);
  const size_t n_seqpos = (size_t)h_seq_off_[n];
  ScanPos pos(n_seqpos, n);
  const bool no_rss = (flags_ & ELEMDP_NO_RSS) != 0;
  HelixArgs ha;
  std::memset(&ha, 0, sizeof(ha));
  if (structure) {
    stems.upload_cleared(d_hx_soff_, {{&d_hx_si_, &stems.i}, {&d_hx_sd_, &s_d}, {&d_hx_slen_, &stems.label}}, d_hx_sp_, st_);
    ha.soff = d_hx_soff_.as<int64_t>(); ha.s_p = d_hx_sp_.as<double>();
    ha.s_i = d_hx_si_.as<int32_t>(); ha.s_d = d_hx_sd_.as<int32_t>(); ha.s_len = d_hx_slen_.as<int32_t>();
  }
  HIP_OK(hipEventRecord(ev_[1], st_));
  ha.plans = plan_.d_plans.as<SeqPlan>();
  ha.seq_out = d_seq_out_.as<double>(); ha.out_stride = out_stride_;
  ha.okbits = d_okbits1_.as<uint32_t>();
  ha.max_len = max_len; ha.min_len = min_len;
  ha.no_rss = no_rss ? 1 : 0;
  ha.min_prob = min_prob;
  const size_t pcells = helix_units_cap(Lmax_, Wmax_);
  ha.p_stride = pcells; ha.u_stride = pcells;
  if (want_list) {   // staging ranges: a sequence's list holds at most max_len - min_len + 1 entries per kept cell
    const StagedList::Staging sl = helices_.begin(plan_.d_plans.as<SeqPlan>(), d_okbits1_.as<uint32_t>(), n, max_len - min_len + 1, st_);
    ha.koff = sl.koff; ha.cnt = sl.cnt;
    ha.st_i = sl.st_i; ha.st_j = sl.st_j; ha.st_k = sl.st_k; ha.st_h = sl.st_v[0];
  }
  const bool work = want_list || structure;   // (else: nothing to compute, no sweep)
  auto at_slot = [&](HelixArgs& hk, size_t slot0) {
    hk.n_units = slot_scratch<int32_t>(d_hx_nu_, 1, slot0);
    hk.ui = slot_scratch<int32_t>(d_hx_ui_, pcells, slot0);
    hk.ud = slot_scratch<int32_t>(d_hx_ud_, pcells, slot0);
    hk.nlen = slot_scratch<int32_t>(d_hx_nlen_, pcells, slot0);
    hk.X = slot_scratch<double>(d_hx_X_, pcells * (size_t)max_len, slot0);
  };
  int n_flagged = 0;
  if (work) {
    PairArgs pa = pair_batch_args();
    pa.p_stride = pcells;
    n_flagged = scan_both_forms(pos, [&](LinArgs& a) {
      if (a.lay.shadow >= 0 || a.lay.S != lay_.S) throw std::logic_error("helix_posteriors: the scan sweeps another automaton than the engine's");
      at_slot(ha, 0);
      ha.P = slot_scratch<double>(d_hx_P_, pcells);
      pair_plane_fields(pa, a);
      ha.skip_flagged = 1;
    }, [&](const LinArgs& ak, size_t slot0, int G, int Lg, int Wg, hipStream_t st) {
      HIP_OK(launch_lin_world_group(ak, G, Lg, Wg, st));
      HelixArgs hk = ha;
      hk.idx = ak.grp;
      at_slot(hk, slot0);
      if (!no_rss) {   // (else the band tables are not read: no units, the stems keep their 0)
        if (want_list) {
          PairArgs pk = pa;
          pk.idx = ak.grp;
          pk.band_in = ak.band_in; pk.band_out = ak.band_out; pk.zs = ak.zs + ak.world;
          pk.P = slot_scratch<double>(d_hx_P_, pcells, slot0);
          hk.P = pk.P;
          HIP_OK(launch_pair_cells(pk, G, (Lg + 1) * (Wg + 1), st));
          HIP_OK(launch_helix_units(hk, G, st));
        }
        HIP_OK(launch_helix_chains(ak, hk, G, (Lg + 1) * (Wg + 1), st));
      }
      if (want_list) HIP_OK(launch_helix_seq(hk, G, st));
    },
    // ---- the log-space form, in chunks of at most as many sequences as the table slots hold (the scratch is bounded by the chunk)
    [&](DpArgs& d, int n_blocks, int n_log) {
      at_slot(ha, 0);
      d_hx_vec_.alloc(8 * 2 * (size_t)d.lay.S * kThreads * (size_t)std::max(n_blocks, 1));
      d.hlx = ha;
      d.hlx.vec = d_hx_vec_.as<double>();
      return log_chunk(n_blocks, n_log);
    }, [&](const int32_t* idx, int C) {
      HelixArgs hk = ha;
      hk.idx = idx;
      hk.skip_flagged = 0;
      hk.no_rss = 0;   // (the fused kernel wrote the number of units of every sequence of the launch: 0 without secondary structure)
      if (want_list) HIP_OK(launch_helix_seq(hk, C, st_));
    });
  }
  finish_call(n_flagged, [&] {
    if (want_list) helices_.finish(st_); else helices_.set_empty();   // the list in (sequence, i, j, len) order
    stems.download(d_hx_sp_, st_);
  });
  if (structure) stems.write(h_seq_off_, n, stem_len, stem_prob);
  if (n_entries) *n_entries = helices_.count();
}

void Engine::helix_list(int32_t* seq, int32_t* i, int32_t* j, int32_t* len, double* p, int64_t cap) {
  require_device();
  DeviceGuard dg(device_);
  helices_.fetch(seq, i, j, p, nullptr, len, cap);
}

// ---- loop posteriors (loop_rules.h).  The host parses the loops of the caller's structures.  The scan's first sum
// pass per group, then on the group's table slots, before the next group of the stream reuses them: P of every cell (k4_pairs), the
// units -- the kept cells whose P reaches the bound -- (k_helix_units: one compaction for both calls), their columns H, S, M
// (k_loop_unary), the two-loop values of their items and B, I (k_loop_items), the loops of the structures (k_loop_struct), and the
// counts and the entries of both lists into the staging ranges (k_loop_seq).  The log-space form -- the fused scan kernel up to its
// first outside pass, then the same rule on its dense tables -- for the sequences that leave the double range and under pipeline 3,
// with k_loop_seq behind the launch.  Then the batch lists (LoopLists, staged_list.h).  The bound is loop_pick_bound(min_prob); where
// the counts are asked for it is 0, since they cover every kept cell.  Every buffer is the call's own: leaves the lists of the last
// pair, conditional, stem and helix call alone.
void Engine::loop_posteriors(const double* x, int n_param_in, double min_prob, double* counts, int64_t* n_closing, int64_t* n_two,
                             const char* structure, int32_t* loop_type, double* loop_prob) {
  require_device();
  DeviceGuard dg(device_);
  if (!(min_prob >= 0.)) throw ArgError("loop_posteriors: min_prob must be >= 0");
  if (structure && !loop_type && !loop_prob) throw ArgError("loop_posteriors: a structure needs loop_type or loop_prob");
  if (n_seq_ <= 0) throw StateError("loop_posteriors before load_batch");
  const int n = n_seq_;
  const bool want_list = min_prob < HUGE_VAL;
  // the loops of every sequence: (type, i, d, k, l) of every pair, sequences and 5' ends in increasing order; the label is the type
  StructItems loops;
  std::vector<int32_t> s_d, s_k, s_l;
  if (structure)
    loops.parse("loop_posteriors", structure, h_seq_off_, n, [&](const int32_t* mate, int L) { structure_loops(mate, L, &loops.label, &loops.i, &s_d, &s_k, &s_l); });
  loops_.invalidate();
  if (streaming_) {
    stream_listed(&Engine::loops_, n_param_in, [&](int c0, size_t at, Engine& e) {
      e.loop_posteriors(x, n_param_in, min_prob, counts ? counts + (size_t)LOOP_COLS * c0 : nullptr, nullptr, nullptr,
                        structure ? structure + at : nullptr, loop_type ? loop_type + at : nullptr, loop_prob ? loop_prob + at : nullptr);
    });
    if (n_closing) *n_closing = loops_.n_closing();
    if (n_two) *n_two = loops_.n_two();
    return;
  }
  require_resident("loop_posteriors", n_param_in);
  upload_params(x, lay_, false);
  const size_t n_seqpos = (size_t)h_seq_off_[n];
  ScanPos pos(n_seqpos, n);
  const bool no_rss = (flags_ & ELEMDP_NO_RSS) != 0;
  LoopArgs la;
  std::memset(&la, 0, sizeof(la));
  if (structure) {
    loops.upload_cleared(d_lp_soff_, {{&d_lp_st_, &loops.label}, {&d_lp_si_, &loops.i}, {&d_lp_sd_, &s_d}, {&d_lp_sk_, &s_k}, {&d_lp_sl_, &s_l}},
                         d_lp_sp_, st_);
    la.soff = d_lp_soff_.as<int64_t>(); la.s_p = d_lp_sp_.as<double>();
    la.s_type = d_lp_st_.as<int32_t>(); la.s_i = d_lp_si_.as<int32_t>(); la.s_d = d_lp_sd_.as<int32_t>();
    la.s_k = d_lp_sk_.as<int32_t>(); la.s_l = d_lp_sl_.as<int32_t>();
  }
  HIP_OK(hipEventRecord(ev_[1], st_));
  const PlanArrays pa_ = plan_.arrays();
  la.plans = plan_.d_plans.as<SeqPlan>();
  la.seq_out = d_seq_out_.as<double>(); la.out_stride = out_stride_;
  la.okbits = d_okbits1_.as<uint32_t>();
  la.no_rss = no_rss ? 1 : 0;
  la.want_units = want_list || counts ? 1 : 0;
  la.min_prob = min_prob;
  la.bound = counts ? 0. : loop_pick_bound(min_prob);
  la.items = pa_.items; la.by_outer_off = pa_.by_outer_off; la.item_in = pa_.item_in;
  const size_t pcells = loop_units_cap(Lmax_, Wmax_);
  size_t items_max = 1;
  for (const SeqPlan& p : plan_.h) items_max = std::max(items_max, (size_t)p.n_items);
  la.p_stride = pcells; la.u_stride = pcells; la.t_stride = items_max;
  if (counts) {
    d_lp_counts_.alloc(8 * (size_t)LOOP_COLS * n);
    HIP_OK(hipMemsetAsync(d_lp_counts_.as<void>(), 0, 8 * (size_t)LOOP_COLS * n, st_));
    la.counts = d_lp_counts_.as<double>();
  }
  // staging ranges: a closing entry per kept cell, a two-loop entry per item at the most
  if (want_list) loops_.begin(plan_.d_plans.as<SeqPlan>(), d_okbits1_.as<uint32_t>(), n, plan_.n_items, &la, st_);
  const bool work = la.want_units || structure;   // (else: nothing to compute, no sweep)
  auto at_slot = [&](LoopArgs& lk, size_t slot0) {
    lk.P = slot_scratch<double>(d_lp_P_, pcells, slot0);
    lk.n_units = slot_scratch<int32_t>(d_lp_nu_, 1, slot0);
    lk.ui = slot_scratch<int32_t>(d_lp_ui_, pcells, slot0);
    lk.ud = slot_scratch<int32_t>(d_lp_ud_, pcells, slot0);
    lk.cols = slot_scratch<double>(d_lp_cols_, pcells * (size_t)LOOP_COLS, slot0);
    lk.T = slot_scratch<double>(d_lp_T_, items_max, slot0);
  };
  int n_flagged = 0;
  if (work) {
    PairArgs pa = pair_batch_args();
    pa.p_stride = pcells;
    n_flagged = scan_both_forms(pos, [&](LinArgs& a) {
      if (a.lay.shadow >= 0 || a.lay.S != lay_.S) throw std::logic_error("loop_posteriors: the scan sweeps another automaton than the engine's");
      at_slot(la, 0);
      pair_plane_fields(pa, a);
      la.skip_flagged = 1;
    }, [&](const LinArgs& ak, size_t slot0, int G, int Lg, int Wg, hipStream_t st) {
      HIP_OK(launch_lin_world_group(ak, G, Lg, Wg, st));
      LoopArgs lk = la;
      lk.idx = ak.grp;
      at_slot(lk, slot0);
      if (!no_rss) {   // (else the band tables are not read: no units, the loops keep their 0)
        if (la.want_units) {
          PairArgs pk = pa;
          pk.idx = ak.grp;
          pk.band_in = ak.band_in; pk.band_out = ak.band_out; pk.zs = ak.zs + ak.world;
          pk.P = lk.P;
          HIP_OK(launch_pair_cells(pk, G, (Lg + 1) * (Wg + 1), st));
          HIP_OK(launch_helix_units(loop_unit_pick(lk, counts ? 0. : min_prob), G, st));
          HIP_OK(launch_loop_unary(ak, lk, G, (Lg + 1) * (Wg + 1), st));
          HIP_OK(launch_loop_items(ak, lk, G, (Lg + 1) * (Wg + 1), st));
        }
        if (structure) HIP_OK(launch_loop_struct(ak, lk, G, Lg, st));
      }
      if (la.want_units) HIP_OK(launch_loop_seq(lk, G, st));
    },
    // ---- the log-space form, in chunks of at most as many sequences as the table slots hold (the scratch is bounded by the chunk)
    [&](DpArgs& d, int n_blocks, int n_log) {
      at_slot(la, 0);
      d.lop = la;
      return log_chunk(n_blocks, n_log);
    }, [&](const int32_t* idx, int C) {
      LoopArgs lk = la;
      lk.idx = idx;
      lk.skip_flagged = 0;
      lk.no_rss = 0;   // (the fused kernel wrote the number of units of every sequence of the launch: 0 without secondary structure)
      if (la.want_units) HIP_OK(launch_loop_seq(lk, C, st_));
    });
  }
  finish_call(n_flagged, [&] {
    if (want_list) loops_.finish(plan_.d_plans.as<SeqPlan>(), pa_.items, st_); else loops_.set_empty();
    loops.download(d_lp_sp_, st_);
    if (counts) HIP_OK(hipMemcpyAsync(counts, d_lp_counts_.as<void>(), 8 * (size_t)LOOP_COLS * n, hipMemcpyDeviceToHost, st_));
  });
  if (structure) loops.write(h_seq_off_, n, loop_type, loop_prob);
  if (n_closing) *n_closing = loops_.n_closing();
  if (n_two) *n_two = loops_.n_two();
}

void Engine::loop_closing_list(int32_t* seq, int32_t* i, int32_t* j, double* p, double* cols, int64_t cap) {
  require_device();
  DeviceGuard dg(device_);
  loops_.fetch_closing(seq, i, j, p, cols, cap);
}

void Engine::loop_two_list(int32_t* seq, int32_t* i, int32_t* j, int32_t* k, int32_t* l, double* p, int64_t cap) {
  require_device();
  DeviceGuard dg(device_);
  loops_.fetch_two(seq, i, j, k, l, p, cap);
}

// ---- maximum expected accuracy motif alignments and site lists (node_mea_rules.h).  The node pass of
// node_profile, then k_node_mea once over the profile of the whole batch on the engine's stream, behind the last group and the
// log-space form.  The profile goes to the host only where the caller gave a buffer.  Leaves the list of the last pair call alone.
void Engine::node_mea(const double* x, int n_param_in, double gamma, int max_sites, const NodeMeaOut& out) {
  require_device();
  DeviceGuard dg(device_);
  const int M = au_.M(), K = max_sites;
  if (!(gamma > 0.) || !std::isfinite(gamma)) throw ArgError("node_mea: gamma must be finite and > 0");
  if (K < 1 || K > kNodeMeaMaxSites) throw ArgError("node_mea: max_sites must lie in 1 .. 64");
  if (M > kNodeMeaMaxNodes) throw ArgError("node_mea: more than 255 pattern nodes");
  if (streaming_) {
    stream_call(n_param_in, [] {}, [&](int c0, int, Engine& e) {
      const size_t at = (size_t)(h_seq_off_[c0] - h_seq_off_[0]), s0 = (size_t)c0 * K;   // (the chunk's first position / first slot)
      const NodeMeaOut oc{out.profile ? out.profile + (size_t)M * at : nullptr, out.node ? out.node + (size_t)K * at : nullptr,
                          out.n_sites ? out.n_sites + c0 : nullptr, out.start ? out.start + s0 : nullptr,
                          out.end ? out.end + s0 : nullptr, out.score ? out.score + s0 : nullptr, out.conf ? out.conf + s0 : nullptr};
      e.node_mea(x, n_param_in, gamma, K, oc);
    });
    return;
  }
  const int n_flagged = node_profile_device("node_mea", x, n_param_in);
  const int n = n_seq_;
  const size_t n_seqpos = (size_t)h_seq_off_[n], n_slots = (size_t)n * K;
  std::vector<int32_t> lists;
  {
    std::string names(M, ' ');
    for (int m = 0; m < M; ++m) names[m] = au_.node(m);
    node_mea_lists_build(names.data(), M, &lists);
  }
  d_nm_lists_.upload(lists, st_);
  d_nm_bp_.alloc((size_t)M * std::max<size_t>(n_seqpos, 1));
  d_nm_node_.alloc((size_t)K * std::max<size_t>(n_seqpos, 1));
  d_nm_ns_.alloc(4 * (size_t)n);
  d_nm_s0_.alloc(4 * n_slots); d_nm_s1_.alloc(4 * n_slots);
  d_nm_sc_.alloc(8 * n_slots); d_nm_cf_.alloc(8 * n_slots);
  NodeMeaArgs ma;
  std::memset(&ma, 0, sizeof(ma));
  ma.plans = plan_.d_plans.as<SeqPlan>();
  ma.lists = d_nm_lists_.as<int32_t>();
  ma.M = M; ma.max_sites = K; ma.gamma = gamma;
  ma.profile = d_nd_prof_.as<double>();
  ma.bp = d_nm_bp_.as<uint8_t>();
  ma.node = d_nm_node_.as<uint8_t>(); ma.n_sites = d_nm_ns_.as<int32_t>();
  ma.start = d_nm_s0_.as<int32_t>(); ma.end = d_nm_s1_.as<int32_t>();
  ma.score = d_nm_sc_.as<double>(); ma.conf = d_nm_cf_.as<double>();
  HIP_OK(launch_node_mea(ma, n, st_));
  auto fetch = [&](void* dst, const DevBuf& src, size_t bytes) {
    if (dst && bytes) HIP_OK(hipMemcpyAsync(dst, src.as<void>(), bytes, hipMemcpyDeviceToHost, st_));
  };
  finish_call(n_flagged, [&] {   // (its wait: the host vector of the lists goes out of use there at the latest)
    fetch(out.profile, d_nd_prof_, 8 * (size_t)M * n_seqpos);
    fetch(out.node, d_nm_node_, (size_t)K * n_seqpos);
    fetch(out.n_sites, d_nm_ns_, 4 * (size_t)n);
    fetch(out.start, d_nm_s0_, 4 * n_slots); fetch(out.end, d_nm_s1_, 4 * n_slots);
    fetch(out.score, d_nm_sc_, 8 * n_slots); fetch(out.conf, d_nm_cf_, 8 * n_slots);
  });
}


// ---- stochastic samples of derivations (sample_rules.h).  The inside sweeps of the scan's first sum pass per group
// (launch_lin_scan_group, SCAN_PASS_INSIDE: no outside pass) and k_sample on the group's slots right behind them, before the next group of the
// stream reuses them; the log-space form in the fused scan kernel for the sequences the range check flags.
void Engine::sample_structures(const double* x, int n_param_in, int n_samples, uint64_t seed, int64_t index_base,
                               const SampleOut& out) {
  require_device();
  DeviceGuard dg(device_);
  if (n_samples <= 0) throw ArgError("sample: n_samples must be > 0");
  if (n_node() > 255) throw ArgError("sample: more than 255 motif nodes do not fit the node bytes");
  if (streaming_) { stream_samples(x, n_param_in, n_samples, seed, index_base, out); return; }
  require_resident("sample", n_param_in);
  upload_params(x, lay_, false);
  const int n = n_seq_;
  const size_t n_seqpos = (size_t)h_seq_off_[n];
  const size_t n_bytes = (size_t)n_samples * n_seqpos;
  const int cap = sample_stack_cap(Lmax_);
  d_sm_rss_.alloc(std::max<size_t>(n_bytes, 1)); d_sm_node_.alloc(std::max<size_t>(n_bytes, 1));
  d_sm_logp_.alloc(8 * (size_t)n * n_samples); d_sm_status_.alloc(4 * (size_t)n);
  HIP_OK(hipEventRecord(ev_[1], st_));
  SampleArgs sa;
  std::memset(&sa, 0, sizeof(sa));
  sa.n_samples = n_samples; sa.seed = seed; sa.index_base = index_base;
  sa.rss = d_sm_rss_.as<char>(); sa.node = d_sm_node_.as<uint8_t>(); sa.logp = d_sm_logp_.as<double>();
  sa.status = d_sm_status_.as<int32_t>();
  sa.stack_cap = cap;
  sa.world = opt_world_;   // (the terminal draw of sample_rules.h)
  const ScanPos pos(n_seqpos, n);
  const int n_flagged = scan_both_forms(pos, [&](LinArgs&) {
    sa.stack_lanes = std::min(n_samples, kSampleLanes);
    sa.stack = slot_scratch<TraceFrame>(d_sm_stack_, (size_t)sa.stack_lanes * cap);
  }, [&](const LinArgs& ak, size_t slot0, int G, int Lg, int Wg, hipStream_t st) {
    HIP_OK(launch_lin_scan_group(ak, G, Lg, Wg, SCAN_PASS_INSIDE, st));
    SampleArgs sk = sa;
    sk.stack = slot_scratch<TraceFrame>(d_sm_stack_, (size_t)sa.stack_lanes * cap, slot0);
    HIP_OK(launch_sample(ak, sk, G, st));
  },
  // ---- the log-space form: the fused scan kernel stops after its inside pass and draws the samples on its own slot before it
  // takes the next sequence (stacks per workgroup, not per sequence)
  [&](DpArgs& d, int n_blocks, int n_log) {
    const int lanes = std::min(n_samples, kThreads);
    d_sm_stack_.alloc(sizeof(TraceFrame) * (size_t)n_blocks * lanes * cap);
    d.smp = sa;
    d.smp.stack = d_sm_stack_.as<TraceFrame>();
    d.smp.stack_lanes = lanes;
    return n_log;
  }, [](const int32_t*, int) {});
  finish_call(n_flagged);
  if (out.rss && n_bytes) HIP_OK(hipMemcpy(out.rss, d_sm_rss_.as<void>(), n_bytes, hipMemcpyDeviceToHost));
  if (out.node && n_bytes) HIP_OK(hipMemcpy(out.node, d_sm_node_.as<void>(), n_bytes, hipMemcpyDeviceToHost));
  if (out.logp) HIP_OK(hipMemcpy(out.logp, d_sm_logp_.as<void>(), 8 * (size_t)n * n_samples, hipMemcpyDeviceToHost));
  if (out.status) HIP_OK(hipMemcpy(out.status, d_sm_status_.as<void>(), 4 * (size_t)n, hipMemcpyDeviceToHost));
}

void Engine::stream_samples(const double* x, int n_param_in, int n_samples, uint64_t seed, int64_t index_base,
                            const SampleOut& out) {
  stream_call(n_param_in, [] {}, [&](int c0, int, Engine& e) {
    const int64_t at = (h_seq_off_[c0] - h_seq_off_[0]) * (int64_t)n_samples;   // (the chunk's first sample byte)
    const SampleOut oc{out.rss ? out.rss + at : nullptr, out.node ? out.node + at : nullptr,
                       out.logp ? out.logp + (size_t)c0 * n_samples : nullptr, out.status ? out.status + c0 : nullptr};
    e.sample_structures(x, n_param_in, n_samples, seed, index_base + c0, oc);
  });
}


// ---- shuffled negatives (host) ------------------------------------------------------------------------------------
// k-let preserving shuffle by a random Euler tour (uShuffle): vertices = distinct (k-1)-lets in order of first
// appearance, edges = consecutive lets; a random arborescence towards the last let (Wilson), the remaining out-edges of
// every vertex permuted, then the walk from the first let.  The calls of rand() -- `rand() % n` in exactly this order --
// are what makes the result identical to the reference's for the same srand() seed.
namespace {
void kmer_shuffle(const uint8_t* s, int l, int k, uint8_t* t) {
  auto rnd = [](int n) { return (int)(static_cast<long>(std::rand()) % n); };
  if (k >= l) { std::copy(s, s + l, t); return; }
  if (k <= 1) {
    std::copy(s, s + l, t);
    for (int i = l - 1; i > 0; --i) std::swap(t[i], t[rnd(i + 1)]);
    return;
  }
  const int n_lets = l - k + 2;
  std::vector<int> let_vertex(n_lets), first_pos;   // vertex id of every let; first position of every vertex
  for (int i = 0; i < n_lets; ++i) {
    int v = -1;
    for (size_t u = 0; u < first_pos.size() && v < 0; ++u)
      if (std::equal(s + first_pos[u], s + first_pos[u] + (k - 1), s + i)) v = (int)u;
    if (v < 0) { v = (int)first_pos.size(); first_pos.push_back(i); }
    let_vertex[i] = v;
  }
  const int nv = (int)first_pos.size(), root = let_vertex[n_lets - 1];
  std::vector<std::vector<int>> succ(nv);
  for (int i = 0; i + 1 < n_lets; ++i) succ[let_vertex[i]].push_back(let_vertex[i + 1]);
  std::vector<char> intree(nv, 0);
  std::vector<int> next(nv, 0);
  intree[root] = 1;
  for (int i = 0; i < nv; ++i) {
    int u = i;
    while (!intree[u]) { next[u] = rnd((int)succ[u].size()); u = succ[u][next[u]]; }
    u = i;
    while (!intree[u]) { intree[u] = 1; u = succ[u][next[u]]; }
  }
  auto permute = [&](std::vector<int>& a, int n) { for (int i = n - 1; i > 0; --i) std::swap(a[i], a[rnd(i + 1)]); };
  for (int i = 0; i < nv; ++i) {
    std::vector<int>& a = succ[i];
    const int n = (int)a.size();
    if (i != root) { std::swap(a[n - 1], a[next[i]]); permute(a, n - 1); }
    else permute(a, n);
  }
  std::copy(s, s + (k - 1), t);
  std::vector<int> walked(nv, 0);
  int u = 0, pos = k - 1;
  while (walked[u] < (int)succ[u].size()) {
    const int v = succ[u][walked[u]];
    t[pos++] = s[first_pos[v] + k - 2];
    ++walked[u];
    u = v;
  }
}
}  // namespace

}  // namespace elemdp

// =================================================================================================
// C ABI
// =================================================================================================
struct elemdp_handle { elemdp::Engine* e; };

namespace {
int fail(const std::exception& ex) {
  elemdp::g_error = ex.what();
  if (dynamic_cast<const elemdp::HipError*>(&ex)) {
    if (elemdp::g_error.find("no HIP device") != std::string::npos) return ELEMDP_ENODEV;
    return ELEMDP_EHIP;
  }
  if (dynamic_cast<const elemdp::StateError*>(&ex)) return ELEMDP_ESTATE;
  if (dynamic_cast<const std::bad_alloc*>(&ex)) return ELEMDP_ENOMEM;
  return ELEMDP_EINVAL;
}
}  // namespace

#define ELEMDP_TRY try {
#define ELEMDP_CATCH                        \
  return ELEMDP_OK;                         \
  }                                         \
  catch (const std::exception& ex) {        \
    return fail(ex);                        \
  }

extern "C" {

const char* elemdp_last_error(void) { return elemdp::g_error.c_str(); }
int elemdp_abi_version(void) { return ELEMDP_ABI_VERSION; }
int elemdp_set_data_dir(const char* dir) {
  elemdp::g_data_dir = dir ? dir : "";
  return ELEMDP_OK;
}

int elemdp_create(const elemdp_model_desc* desc, elemdp_handle** out) {
  ELEMDP_TRY
  if (!desc || !out) throw elemdp::ArgError("elemdp_create: null argument");
  *out = nullptr;
  std::unique_ptr<elemdp::Engine> e(new elemdp::Engine(*desc));
  *out = new elemdp_handle{e.release()};
  ELEMDP_CATCH
}
int elemdp_destroy(elemdp_handle* h) {
  if (h) { delete h->e; delete h; }
  return ELEMDP_OK;
}
int elemdp_n_param(const elemdp_handle* h) { return h ? h->e->n_param() : ELEMDP_EINVAL; }
int elemdp_n_state(const elemdp_handle* h) { return h ? h->e->n_state() : ELEMDP_EINVAL; }
int elemdp_n_node(const elemdp_handle* h) { return h ? h->e->n_node() : ELEMDP_EINVAL; }

int elemdp_initial_params(const elemdp_handle* h, double lambda_init, double* x, int32_t n_param) {
  ELEMDP_TRY
  if (!h || !x || n_param != h->e->n_param()) throw elemdp::ArgError("elemdp_initial_params: bad argument");
  const elemdp::Automaton& au = h->e->automaton();
  int k = 0;
  for (int r = 0; r < au.n_rows(); ++r)
  {
    // log-softmax of an all-zero score row, summed the way ProfileHMM::calc_theta does (profile_hmm.hpp:103-111)
    double tot = -INFINITY;
    for (int c = 0; c < au.row_width(r); ++c) tot = (tot == -INFINITY) ? 0. : tot + std::log1p(std::exp(0. - tot));
    for (int c = 0; c < au.row_width(r); ++c) x[k++] = h->e->softmax() ? 0. : 0. - tot;
  }
  x[k++] = lambda_init;
  x[k++] = lambda_init;
  ELEMDP_CATCH
}
int elemdp_describe(const elemdp_handle* h, char* buf, int32_t cap) {
  if (!h || !buf) return ELEMDP_EINVAL;
  std::string s = h->e->automaton().to_json();
  {   // sizes of the flattened automaton the kernels sweep (pruned as the options say): for inspection and tests
    const elemdp::AutomatonLayout& L = h->e->layout();
    char extra[320];
    std::snprintf(extra, sizeof(extra), ", \"layout\": {\"S\": %d, \"n_ap\": %d, \"n_quad\": %d, \"n_split\": %d, \"n_lane\": %d, \"n_front\": %d, \"fp_ok\": %d, "
                  "\"shadow\": %d, \"n_ints\": %d, \"fast_blob_in\": %d, \"fast_blob_out\": %d}}",
                  L.S, L.n_ap, L.n_quad, L.n_split, L.n_lane, L.n_front, L.fp_ok, L.shadow, L.n_ints, L.fb_in_n, L.fb_out_n);
    const size_t close = s.rfind('}');
    if (close != std::string::npos) s = s.substr(0, close) + extra;
  }
  if ((int)s.size() + 1 > cap) return ELEMDP_EINVAL;
  std::memcpy(buf, s.c_str(), s.size() + 1);
  return (int)s.size();
}
int elemdp_set_option(elemdp_handle* h, const char* key, double value) {
  ELEMDP_TRY
  if (!h || !key) throw elemdp::ArgError("elemdp_set_option: null argument");
  h->e->set_option(key, value);
  ELEMDP_CATCH
}

int elemdp_load_batch(elemdp_handle* h, const uint8_t* seq_codes, const int32_t* seq_off, const uint8_t* qual,
                      const int32_t* qual_off, const char* fix_rss, int32_t n_seq) {
  ELEMDP_TRY
  if (!h) throw elemdp::ArgError("null handle");
  h->e->load_batch(seq_codes, seq_off, qual, qual_off, fix_rss, n_seq);
  ELEMDP_CATCH
}
int elemdp_load_batch_constrained(elemdp_handle* h, const uint8_t* seq_codes, const int32_t* seq_off, const uint8_t* qual,
                                  const int32_t* qual_off, const char* constraint, int32_t n_seq) {
  ELEMDP_TRY
  if (!h) throw elemdp::ArgError("null handle");
  h->e->load_batch(seq_codes, seq_off, qual, qual_off, nullptr, n_seq, constraint);
  ELEMDP_CATCH
}
int elemdp_constraint_mask_host(const uint8_t* kept, const uint8_t* seq, const char* constraint, int32_t L, int32_t W, int32_t flags,
                                uint8_t* kept_out, uint8_t* unp_out) {
  ELEMDP_TRY
  if (!kept || !seq || !constraint || !kept_out || !unp_out || L < 1 || W < 0 || W > L)
    throw elemdp::ArgError("elemdp_constraint_mask_host: bad argument");
  if ((int64_t)std::strlen(constraint) != L)
    throw elemdp::ArgError("constraint of sequence 0: " + std::to_string(std::strlen(constraint)) + " characters for a sequence of " + std::to_string(L));
  const int min_span = (flags & ELEMDP_DBG_NO_TURN) ? 1 : 5;
  std::vector<uint8_t> cls(L);
  std::vector<int32_t> partner(L), enc(L);
  const auto pair_ok = [&](int i, int j) { return elemdp::canonical_pair(seq, L, W, min_span, i, j - i + 1); };
  const std::string err = elemdp::constraint_derive(constraint, L, 0, pair_ok, cls.data(), partner.data(), enc.data(), unp_out, nullptr);
  if (!err.empty()) throw elemdp::ArgError(err);
  const int64_t nc = (int64_t)(L + 1) * (W + 1);
  const int nword = (int)((nc + 31) / 32);
  const elemdp::ConsView c{cls.data(), partner.data(), enc.data()};
  for (int w = 0; w < nword; ++w) {
    uint32_t in = 0;
    for (int k = 0; k < 32 && (int64_t)w * 32 + k < nc; ++k) in |= (kept[(size_t)w * 32 + k] ? 1u : 0u) << k;
    const uint32_t out = elemdp::cons_word(c, L, W, w, in);
    for (int k = 0; k < 32 && (int64_t)w * 32 + k < nc; ++k) kept_out[(size_t)w * 32 + k] = (out >> k) & 1u;
  }
  ELEMDP_CATCH
}
int elemdp_batch_bpp_eff(elemdp_handle* h, double* bpp_eff, int32_t n_seq) {
  ELEMDP_TRY
  if (!h || !bpp_eff || n_seq != h->e->n_seq()) throw elemdp::ArgError("elemdp_batch_bpp_eff: bad argument");
  if (!h->e->bpp_eff_known()) throw elemdp::StateError("elemdp_batch_bpp_eff: the batch is streamed in chunks and not every chunk has been loaded yet (evaluate or scan first)");
  for (int k = 0; k < n_seq; ++k) bpp_eff[k] = h->e->plans()[k].bpp_eff;
  ELEMDP_CATCH
}
int elemdp_batch_pairs(elemdp_handle* h, int32_t seq_index, uint8_t* kept, double* lnbpp, int32_t cap) {
  ELEMDP_TRY
  if (!h || !kept) throw elemdp::ArgError("elemdp_batch_pairs: null argument");
  h->e->batch_pairs(seq_index, kept, lnbpp, cap);
  ELEMDP_CATCH
}

int elemdp_useful_mask(elemdp_handle* h, int32_t seq_index, uint8_t* mask, int32_t cap) {
  ELEMDP_TRY
  if (!h || !mask) throw elemdp::ArgError("elemdp_useful_mask: null argument");
  h->e->useful_mask(seq_index, mask, cap);
  ELEMDP_CATCH
}
int elemdp_live_blocks(elemdp_handle* h, int32_t seq_index, int32_t* counts, void* records, int32_t stride, int32_t* cpb_cap,
                       int32_t* taken) {
  ELEMDP_TRY
  if (!h || !counts || !records || !cpb_cap) throw elemdp::ArgError("elemdp_live_blocks: null argument");
  h->e->live_blocks(seq_index, counts, records, stride, cpb_cap, taken);
  ELEMDP_CATCH
}
int elemdp_live_blocks_inside(elemdp_handle* h, int32_t seq_index, int32_t* counts, void* records, int32_t stride, int32_t* cpb_cap,
                              int32_t* taken) {
  ELEMDP_TRY
  if (!h || !counts || !records || !cpb_cap) throw elemdp::ArgError("elemdp_live_blocks_inside: null argument");
  h->e->live_blocks(seq_index, counts, records, stride, cpb_cap, taken, true);
  ELEMDP_CATCH
}
int elemdp_live_blocks_host_bits(const uint8_t* mask, int32_t L, int32_t W, int32_t cpb, int32_t cap, int32_t bits, int32_t* counts,
                                 void* records, int32_t stride) {
  if (!mask || !counts || !records || L < 0 || W < 0 || W > L || cpb < 1 || cap < cpb || cap > elemdp::kLiveSpanMax ||
      stride < (L + cpb) / cpb || bits < 1 || bits > 255)
    return ELEMDP_EINVAL;
  elemdp::live_blocks_host(mask, L, W, cpb, cap, counts, static_cast<elemdp::LiveBlock*>(records), stride, bits);
  return ELEMDP_OK;
}
int elemdp_live_blocks_host(const uint8_t* mask, int32_t L, int32_t W, int32_t cpb, int32_t cap, int32_t* counts, void* records,
                            int32_t stride) {
  if (!mask || !counts || !records || L < 0 || W < 0 || W > L || cpb < 1 || cap < cpb || cap > elemdp::kLiveSpanMax ||
      stride < (L + cpb) / cpb)
    return ELEMDP_EINVAL;
  elemdp::live_blocks_host(mask, L, W, cpb, cap, counts, static_cast<elemdp::LiveBlock*>(records), stride);
  return ELEMDP_OK;
}
int elemdp_useful_mask_host(const uint8_t* kept, const uint8_t* unp, int32_t L, int32_t W, int32_t max_iloop, int32_t flags,
                            uint8_t* mask) {
  if (!kept || !mask || L < 0 || W < 0 || W > L || max_iloop < 0) return ELEMDP_EINVAL;
  elemdp::useful_mask_host(kept, unp, L, W, max_iloop, (flags & ELEMDP_DBG_NO_TURN) ? 4 : 10, (flags & ELEMDP_NO_ENERGY) != 0, mask);
  return ELEMDP_OK;
}
int elemdp_pair_terms(elemdp_handle* h, int32_t seq_index, uint64_t* ha_rows, uint64_t* h1_stems, int32_t cap) {
  ELEMDP_TRY
  if (!h || !ha_rows || !h1_stems) throw elemdp::ArgError("elemdp_pair_terms: null argument");
  h->e->pair_terms(seq_index, ha_rows, h1_stems, cap);
  ELEMDP_CATCH
}
int elemdp_pair_terms_host(const uint8_t* mask, const uint8_t* kept, int32_t L, int32_t W, uint64_t* ha_rows, uint64_t* h1_stems) {
  if (!mask || !kept || !ha_rows || !h1_stems || L < 0 || W < 0 || W > L || W > elemdp::kPairTermsMaxW) return ELEMDP_EINVAL;
  static_assert(sizeof(uint64_t) == sizeof(unsigned long long), "the words of the plan");
  elemdp::pair_terms_host(mask, kept, L, W, reinterpret_cast<unsigned long long*>(ha_rows), reinterpret_cast<unsigned long long*>(h1_stems));
  return ELEMDP_OK;
}

int elemdp_partial_len(const elemdp_handle* h) { return h ? h->e->partial_len() : ELEMDP_EINVAL; }
int elemdp_train_partial(elemdp_handle* h, const double* x, int32_t n_param, void* partial, int32_t partial_is_device) {
  ELEMDP_TRY
  if (!h || !x || !partial) throw elemdp::ArgError("elemdp_train_partial: null argument");
  h->e->train_partial(x, n_param, partial, partial_is_device != 0);
  ELEMDP_CATCH
}
int elemdp_train_finish(elemdp_handle* h, const double* reduced, double* fn, double* gr, double* sum_eff,
                        int32_t* n_skipped) {
  ELEMDP_TRY
  if (!h || !reduced) throw elemdp::ArgError("elemdp_train_finish: null argument");
  h->e->train_finish(reduced, fn, gr, sum_eff, n_skipped);
  ELEMDP_CATCH
}
int elemdp_set_finish_params(elemdp_handle* h, const double* x, int32_t n_param) {
  ELEMDP_TRY
  if (!h || !x || n_param != h->e->n_param()) throw elemdp::ArgError("elemdp_set_finish_params: bad argument");
  h->e->set_theta_from(x);
  ELEMDP_CATCH
}
int elemdp_train_eval(elemdp_handle* h, const double* x, int32_t n_param, double* fn, double* gr, double* sum_eff,
                      int32_t* n_skipped) {
  ELEMDP_TRY
  if (!h || !x) throw elemdp::ArgError("elemdp_train_eval: null argument");
  std::vector<double> partial(h->e->partial_len());
  h->e->train_partial(x, n_param, partial.data(), false, true);   // (summed over the ranks when a communicator is set)
  h->e->train_finish(partial.data(), fn, gr, sum_eff, n_skipped);
  ELEMDP_CATCH
}
int elemdp_comm_unique_id(void* id_out) {
  ELEMDP_TRY
  if (!id_out) throw elemdp::ArgError("elemdp_comm_unique_id: null argument");
  elemdp::Rccl& r = elemdp::Rccl::get();
  if (!r.ok()) throw elemdp::HipError("no HIP device available for the collective: librccl.so could not be loaded");
  elemdp::Rccl::UniqueId uid;
  RCCL_OK(r.GetUniqueId(&uid));
  std::memcpy(id_out, &uid, sizeof(uid));
  ELEMDP_CATCH
}
int elemdp_comm_init(elemdp_handle* h, int32_t rank, int32_t world, const void* id) {
  ELEMDP_TRY
  if (!h) throw elemdp::ArgError("null handle");
  h->e->comm_init(rank, world, id);
  ELEMDP_CATCH
}
int elemdp_comm_destroy(elemdp_handle* h) {
  ELEMDP_TRY
  if (!h) throw elemdp::ArgError("null handle");
  h->e->comm_destroy();
  ELEMDP_CATCH
}
int elemdp_train_seq_stats(elemdp_handle* h, double* out, int32_t n_seq) {
  ELEMDP_TRY
  if (!h || !out) throw elemdp::ArgError("elemdp_train_seq_stats: null argument");
  h->e->seq_stats(out, n_seq);
  ELEMDP_CATCH
}
int elemdp_train_seq_counts(elemdp_handle* h, double* out, int32_t n_seq) {
  ELEMDP_TRY
  if (!h || !out) throw elemdp::ArgError("elemdp_train_seq_counts: null argument");
  h->e->seq_counts(out, n_seq);
  ELEMDP_CATCH
}
int elemdp_debug_tables(elemdp_handle* h, double* inside, double* outside, double* inside_o, double* outside_o,
                        double* ENo, double* ENx, double* EH) {
  ELEMDP_TRY
  if (!h) throw elemdp::ArgError("null handle");
  h->e->debug_tables(inside, outside, inside_o, outside_o, ENo, ENx, EH);
  ELEMDP_CATCH
}
int elemdp_scan(elemdp_handle* h, const double* x, int32_t n_param, elemdp_scan_out* out) {
  ELEMDP_TRY
  if (!h || !x) throw elemdp::ArgError("elemdp_scan: null argument");
  h->e->scan(x, n_param, out);
  ELEMDP_CATCH
}
int elemdp_pair_posteriors(elemdp_handle* h, const double* x, int32_t n_param, double min_prob, int64_t* n_pairs, double* unpaired) {
  ELEMDP_TRY
  if (!h || !x || !n_pairs) throw elemdp::ArgError("elemdp_pair_posteriors: null argument");
  h->e->pair_posteriors(x, n_param, min_prob, n_pairs, unpaired);
  ELEMDP_CATCH
}
int elemdp_pair_mea(elemdp_handle* h, const double* x, int32_t n_param, double min_prob, double gamma, int64_t* n_pairs,
                    double* unpaired, char* structure, double* score) {
  ELEMDP_TRY
  if (!h || !x || !n_pairs) throw elemdp::ArgError("elemdp_pair_mea: null argument");
  const elemdp::Engine::MeaOut mea{gamma, structure, score};
  h->e->pair_posteriors(x, n_param, min_prob, n_pairs, unpaired, &mea);
  ELEMDP_CATCH
}
int elemdp_sample(elemdp_handle* h, const double* x, int32_t n_param, int32_t n_samples, uint64_t seed, int64_t index_base,
                  char* rss, uint8_t* node, double* logp, int32_t* status) {
  ELEMDP_TRY
  if (!h || !x) throw elemdp::ArgError("elemdp_sample: null argument");
  h->e->sample_structures(x, n_param, n_samples, seed, index_base, elemdp::Engine::SampleOut{rss, node, logp, status});
  ELEMDP_CATCH
}
int elemdp_context_profile(elemdp_handle* h, const double* x, int32_t n_param, double* profile) {
  ELEMDP_TRY
  if (!h || !x || !profile) throw elemdp::ArgError("elemdp_context_profile: null argument");
  h->e->context_profile(x, n_param, profile);
  ELEMDP_CATCH
}
int elemdp_accessibility(elemdp_handle* h, const double* x, int32_t n_param, int32_t max_width, double* access) {
  ELEMDP_TRY
  if (!h || !x || !access) throw elemdp::ArgError("elemdp_accessibility: null argument");
  h->e->accessibility(x, n_param, max_width, access);
  ELEMDP_CATCH
}
int elemdp_node_profile(elemdp_handle* h, const double* x, int32_t n_param, double* profile) {
  ELEMDP_TRY
  if (!h || !x || !profile) throw elemdp::ArgError("elemdp_node_profile: null argument");
  h->e->node_profile(x, n_param, profile);
  ELEMDP_CATCH
}
int elemdp_joint_profile(elemdp_handle* h, const double* x, int32_t n_param, double* counts, double* profile) {
  ELEMDP_TRY
  if (!h || !x || !counts) throw elemdp::ArgError("elemdp_joint_profile: null argument");
  h->e->joint_profile(x, n_param, counts, profile);
  ELEMDP_CATCH
}
int elemdp_stem_slots(const elemdp_handle* h, int32_t* node_left, int32_t* node_right, int32_t cap) {
  try {
    if (!h) throw elemdp::ArgError("elemdp_stem_slots: null handle");
    return h->e->stem_slots(node_left, node_right, cap);
  } catch (const std::exception& ex) {
    return fail(ex);
  }
}
int elemdp_stem_profile(elemdp_handle* h, const double* x, int32_t n_param, double min_prob, double* counts, int64_t* n_entries) {
  ELEMDP_TRY
  if (!h || !x || !counts) throw elemdp::ArgError("elemdp_stem_profile: null argument");
  h->e->stem_profile(x, n_param, min_prob, counts, n_entries);
  ELEMDP_CATCH
}
int elemdp_stem_list(elemdp_handle* h, int32_t* seq, int32_t* i, int32_t* j, int32_t* slot, double* q, int64_t cap) {
  ELEMDP_TRY
  if (!h) throw elemdp::ArgError("elemdp_stem_list: null handle");
  h->e->stem_list(seq, i, j, slot, q, cap);
  ELEMDP_CATCH
}
int elemdp_helix_posteriors(elemdp_handle* h, const double* x, int32_t n_param, int32_t max_len, int32_t min_len, double min_prob,
                            int64_t* n_entries, const char* structure, int32_t* stem_len, double* stem_prob) {
  ELEMDP_TRY
  if (!h || !x) throw elemdp::ArgError("elemdp_helix_posteriors: null argument");
  h->e->helix_posteriors(x, n_param, max_len, min_len, min_prob, n_entries, structure, stem_len, stem_prob);
  ELEMDP_CATCH
}
int elemdp_helix_list(elemdp_handle* h, int32_t* seq, int32_t* i, int32_t* j, int32_t* len, double* p, int64_t cap) {
  ELEMDP_TRY
  if (!h) throw elemdp::ArgError("elemdp_helix_list: null handle");
  h->e->helix_list(seq, i, j, len, p, cap);
  ELEMDP_CATCH
}
int elemdp_loop_posteriors(elemdp_handle* h, const double* x, int32_t n_param, double min_prob, double* counts, int64_t* n_closing,
                           int64_t* n_two, const char* structure, int32_t* loop_type, double* loop_prob) {
  ELEMDP_TRY
  if (!h || !x) throw elemdp::ArgError("elemdp_loop_posteriors: null argument");
  h->e->loop_posteriors(x, n_param, min_prob, counts, n_closing, n_two, structure, loop_type, loop_prob);
  ELEMDP_CATCH
}
int elemdp_loop_closing_list(elemdp_handle* h, int32_t* seq, int32_t* i, int32_t* j, double* p, double* cols, int64_t cap) {
  ELEMDP_TRY
  if (!h) throw elemdp::ArgError("elemdp_loop_closing_list: null handle");
  h->e->loop_closing_list(seq, i, j, p, cols, cap);
  ELEMDP_CATCH
}
int elemdp_loop_two_list(elemdp_handle* h, int32_t* seq, int32_t* i, int32_t* j, int32_t* k, int32_t* l, double* p, int64_t cap) {
  ELEMDP_TRY
  if (!h) throw elemdp::ArgError("elemdp_loop_two_list: null handle");
  h->e->loop_two_list(seq, i, j, k, l, p, cap);
  ELEMDP_CATCH
}
int elemdp_node_mea(elemdp_handle* h, const double* x, int32_t n_param, double gamma, int32_t max_sites, double* profile,
                    uint8_t* node, int32_t* n_sites, int32_t* site_start, int32_t* site_end, double* site_score, double* site_conf) {
  ELEMDP_TRY
  if (!h || !x) throw elemdp::ArgError("elemdp_node_mea: null argument");
  h->e->node_mea(x, n_param, gamma, max_sites, elemdp::Engine::NodeMeaOut{profile, node, n_sites, site_start, site_end, site_score, site_conf});
  ELEMDP_CATCH
}
int elemdp_pair_conditional(elemdp_handle* h, const double* x, int32_t n_param, double min_prob, double gamma, int64_t* n_pairs,
                            double* exist_prob, double* unpaired_motif, double* unpaired_none, char* structure_motif,
                            char* structure_none, double* shift) {
  ELEMDP_TRY
  if (!h || !x || !n_pairs) throw elemdp::ArgError("elemdp_pair_conditional: null argument");
  const elemdp::Engine::CondOut out{gamma, exist_prob, {unpaired_motif, unpaired_none}, {structure_motif, structure_none}, shift};
  h->e->pair_conditional(x, n_param, min_prob, n_pairs, out);
  ELEMDP_CATCH
}
int elemdp_pair_conditional_list(elemdp_handle* h, int32_t* seq, int32_t* i, int32_t* j, double* p_motif, double* p_none, int64_t cap) {
  ELEMDP_TRY
  if (!h) throw elemdp::ArgError("elemdp_pair_conditional_list: null handle");
  h->e->cond_list(seq, i, j, p_motif, p_none, cap);
  ELEMDP_CATCH
}
int elemdp_pair_list(elemdp_handle* h, int32_t* seq, int32_t* i, int32_t* j, double* p, int64_t cap) {
  ELEMDP_TRY
  if (!h) throw elemdp::ArgError("elemdp_pair_list: null handle");
  h->e->pair_list(seq, i, j, p, cap);
  ELEMDP_CATCH
}
int elemdp_last_timing(elemdp_handle* h, double* ms, int32_t n) {
  if (!h || !ms) return ELEMDP_EINVAL;
  for (int k = 0; k < n && k < 3; ++k) ms[k] = h->e->last_ms[k];
  if (n > 3) ms[3] = h->e->last_zeros_kept() ? 1. : 0.;
  if (n > 4) ms[4] = (double)h->e->slots_held();
  if (n > 5) ms[5] = (double)h->e->options_logged();
  return ELEMDP_OK;
}
int elemdp_debug_profile(elemdp_handle* h, double* cycles, int32_t n) {
  if (!h || !cycles) return ELEMDP_EINVAL;
  for (int k = 0; k < n && k < 16; ++k) cycles[k] = k < (int)h->e->last_prof.size() ? (double)h->e->last_prof[k] : 0.;
  return ELEMDP_OK;
}
int elemdp_kmer_shuffle(const uint8_t* codes, int32_t L, int32_t k, int32_t iter_cnt, uint8_t* out) {
  if (!codes || !out || L <= 0) return ELEMDP_EINVAL;
  int cnt = 0;
  for (int i = 0; i < L; ++i) cnt += codes[i] == codes[0];
  std::srand((unsigned)(cnt + iter_cnt));   // motif_trainer.hpp:147
  elemdp::kmer_shuffle(codes, L, k, out);
  return ELEMDP_OK;
}
int elemdp_epoch_permutation(int32_t n, int32_t seed, int32_t* perm) {
  if (n < 0 || (n > 0 && !perm)) return ELEMDP_EINVAL;
  std::vector<int32_t> v(n);
  std::iota(v.begin(), v.end(), 0);
  std::mt19937 m;
  m.seed((unsigned)seed);
  std::shuffle(v.begin(), v.end(), m);   // fastq_io.hpp:117
  std::copy(v.begin(), v.end(), perm);
  return ELEMDP_OK;
}
const char* elemdp_kernel_name(void) { return "k4_out"; }

}  // extern "C"
