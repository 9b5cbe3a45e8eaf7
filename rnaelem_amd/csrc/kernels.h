// kernels.h -- launch interface between the host engine (engine.cpp) and the HIP kernels (kernels.hip).
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>

#include "device_layout.h"
#include "energy_tables.h"
#include "bpp_cand.h"
#include "live_blocks.h"

namespace elemdp {

constexpr int kThreads = 256;  // workgroup size of every kernel (4 waves of 64: one per SIMD of a CU)
constexpr int kPairTermsMaxW = 64;   // the largest span whose pair terms fit a word (PlanArrays::ha_rows)

// device arrays of one plan set (see SeqPlan for the per-sequence bases)
struct PlanArrays {
  int16_t* dmin = nullptr;
  double* e_stack = nullptr; double* e_ext = nullptr; double* e_ml = nullptr; double* e_close = nullptr; double* e_hp = nullptr;
  int32_t* by_outer_off = nullptr; int32_t* by_inner_off = nullptr; int32_t* by_left_off = nullptr; int32_t* by_right_off = nullptr;
  int32_t* cursor = nullptr;  // scratch, one int per CSR offset entry
  LoopItem* items = nullptr;
  uint8_t* item_in = nullptr;
  int32_t* by_inner_idx = nullptr; int32_t* by_left_idx = nullptr; int32_t* by_right_idx = nullptr;
  // copies of the items in the three secondary orders (one dependent load less per term in the outside sweeps)
  LoopItem* items_inner = nullptr; LoopItem* items_left = nullptr; LoopItem* items_right = nullptr;
  // usefulness mask of the train sweeps (plan_rules.h: UB_* bits), one byte per cell at cell_base + d * (L+1) + i; null: every
  // entry counts as useful
  uint8_t* useful = nullptr;
  // live-block lists of the train sweeps (live_blocks.h: LiveBlock, W + 1 headers and the records of every diagonal from
  // SeqPlan::blk_base on); null: a workgroup takes cpb consecutive cells
  LiveBlock* blocks = nullptr;
  // the second set of lists, from the mask bytes without UB_L: the inside sweep behind the loop pre-pass (live_blocks.h)
  LiveBlock* blocks_in = nullptr;
  // pair terms of the outside train sweep (plan_rules.h: ha_rows / h1_stems), one 64-bit word per cell each, indexed like
  // `useful`; null: no words for this plan (W > 64, the mask of all ones, no mask) -- the sweep walks every row and stem
  unsigned long long* ha_rows = nullptr;
  unsigned long long* h1_stems = nullptr;
};

// static per-batch arrays
struct BatchArrays {
  const uint8_t* seq = nullptr;     // base codes
  const double* ws = nullptr;       // position weights
  const uint8_t* unp = nullptr;     // position may be emitted unpaired
  const int32_t* ndot = nullptr;    // FIX_RSS prefix counts (or null)
};

struct PlanKernelArgs {
  const EnergyTables* et;
  BatchArrays b;
  const uint32_t* okbits;
  uint32_t* okbits_end = nullptr;   // the same mask indexed by (end, span): scratch of the plan builder
  SeqPlan* plans;       // plans[first .. first+count)
  int32_t first, count;
  PlanArrays p;
  int32_t no_ene, min_span, fix_rss;
  int32_t m_min = 0;     // smallest span of a multiloop cell (the usefulness mask)
  int32_t ncell_max = 0, nword_max = 0, nitems_max = 0, lmax = 0;   // largest sequence of the set (grid sizes)
  int32_t wmax1 = 0;     // largest W + 1 of the set
  int32_t n_roles = 3;   // 1: only the by_inner order (plan of the BPP filter)
  int32_t sort_roles = 1;   // sort every segment of the role lists by item index (reproducible summation order of the gathers)
  int32_t count_fast = 0;   // loop_tables_finite and no imposed structure: the count pass takes popcounts (count_interior_by_end)
  // live-block lists (launch_live_blocks): cells per block and the span a block may cover; blk_max: three rows of wmax1 ints over
  // the sequences of the set (cleared by the launcher) -- the most blocks of diagonal d, the sum of its blocks, and the sum of
  // the workgroups of cpb consecutive cells that hold a live cell --, then the same three rows for the inside set (p.blocks_in)
  int32_t live_cpb = 0, live_cap = 0;
  int32_t* blk_max = nullptr;
};

// byte offsets of the dynamic LDS regions of the DP kernels
struct LdsLayout {
  int32_t ints, theta, en_o, en_x, eh, zs, ws, post, okbits, dmin, seq, unp, wave_scr, total;
};

enum DpKind : int { DP_TRAIN = 0, DP_BPP = 1, DP_SCAN = 2 };

// ---- stochastic samples of derivations (sample_rules.h, sample_kernels.hip), on the inside tables of launch_lin_scan_group
// (SCAN_PASS_INSIDE), right behind it on the same slots and stream
// (launch_sample), and -- the log-space form -- in the fused scan kernel right after its inside pass (DpArgs::smp).  Batch index n (= grp[g]) with seq_base b and length L writes sample k at
// rss / node + n_samples * b + k * L (L bytes each) and logp[n * n_samples + k]; status[n] is a SampleStatus.
struct TraceFrame;   // (scan_rules.h)
struct SampleArgs {
  int32_t n_samples;
  // option world, in the padding in front of seed: 0 = the mixture, 1 = the terminal is drawn among s0m2, s0m1
  // alone, 2 = s00 alone.  As DpArgs::smp it is also the world of the fused scan kernel's product branches (1 / 2: the first outside
  // pass is seeded with the ari terminals / the nasi terminal alone and normalised with that world's ln Z; no sweep for an empty
  // world, ln Z = -inf: the product's no-parse path)
  int32_t world;
  uint64_t seed;
  int64_t index_base;        // added to the batch index in the generator key
  char* rss; uint8_t* node; double* logp; int32_t* status;
  TraceFrame* stack;         // per slot of the launch: stack_lanes stacks of stack_cap frames, one per walking lane
  int32_t stack_cap, stack_lanes;   // stack_lanes = min(n_samples, lanes of a workgroup)
};
constexpr int kSampleLanes = 64;   // one wave per sequence, one lane per sample

// ---- structural context profiles (ctx_rules.h, ctx_kernels.hip).  A launch covers the G sequences idx[0 .. G) of one group or
// chunk; slot g of the launch owns P, u, h, b + g * c_stride (each [i][d], rows of W+1: the pair posteriors and the per-run
// values of ctx_rules.h) and o + g * o_stride (the exterior column, L values).  The profile of batch index n goes to
// profile + 7 * seq_base, 7 doubles per position in the order O L R H B I M.
constexpr int kCtxCols = 7;
struct CtxArgs {
  const SeqPlan* plans;           // batch plans (batch index)
  const int32_t* idx;             // idx[g] = batch index of the sequence in slot g (launch_ctx_seq)
  const double* seq_out; int32_t out_stride;   // row[4] != 0: the sequence left the double range (the log-space form covers it)
  int32_t skip_flagged;           // 1: leave the sequences flagged in seq_out alone (scaled-linear form)
  double* P; double* u; double* h; double* b; size_t c_stride;
  double* o; size_t o_stride;
  double* profile;
  int32_t no_rss;                 // a model without secondary structure: every position is exterior
};

// ---- posterior motif-node profiles (node_rules.h, node_kernels.hip): the profile of batch index n goes to
// profile + M * seq_base, M doubles per position in node order (0 = 'z' .. M-1 = 'o')
struct NodeArgs {
  const int32_t* lists;           // the transitions by emitted node (node_lists_build)
  int32_t M;                      // pattern nodes
  int32_t rules;                  // NodeRule bits: the rules that take part (all of them unless option node_rules says otherwise)
  int32_t no_rss;                 // a model without secondary structure: rule 8 alone, the band tables are not read
  double* profile;
};

// ---- accessibility (access_rules.h, access_kernels.hip).  A launch covers the G sequences idx[0 .. G) of one group or chunk; slot g
// of the launch owns the four planes T + g * t_stride + term * plane (AccessTerm), rows of U doubles per position 0 .. L.  The result
// of batch index n goes to access + U * seq_base, U doubles per position: the widths 1 .. U.
struct AccessArgs {
  const SeqPlan* plans;           // batch plans (batch index)
  const int32_t* idx;             // idx[g] = batch index of the sequence in slot g (launch_access_seq)
  const double* seq_out; int32_t out_stride;   // row[4] != 0: the sequence left the double range (the log-space form covers it)
  int32_t skip_flagged;           // 1: leave the sequences flagged in seq_out alone (scaled-linear form)
  int32_t U;                      // max_width
  int32_t terms;                  // bit AccessTerm: the terms that take part (all of them unless option access_terms says otherwise)
  int32_t no_rss;                 // a model without secondary structure: every valid window is 1
  double* T; size_t t_stride, plane;
  double* vec;                    // log-space form: two state vectors per thread of a workgroup of the fused scan kernel
  double* access;
};

// ---- joint node-by-context posteriors and emission counts (joint_rules.h, joint_kernels.hip).  Slot g of a launch of the
// scaled-linear form (workgroup b of the fused scan kernel in the log-space form) owns the per-cell scratch X + g * x_stride:
// the sums in(L) G_c / Z of every cell by kind and by emitting node (joint_cell_at).  The profile of batch index n goes to
// profile + 7 M * seq_base, 7 M doubles per position at 7 m + c; its counts to counts + 35 M * n at (7 m + c) 5 + b.
struct JointArgs {
  const SeqPlan* plans;           // batch plans (batch index)
  const int32_t* idx;             // idx[g] = batch index of the sequence in slot g (launch_joint_counts)
  const double* seq_out; int32_t out_stride;   // row[4] != 0: the sequence left the double range (the log-space form covers it)
  int32_t skip_flagged;           // 1: leave the sequences flagged in seq_out alone (scaled-linear form)
  const uint8_t* seq;             // base codes of the batch (BatchArrays::seq)
  const int32_t* lists;           // the transitions by emitted node (node_lists_build), then the slot map at slot_at
  int32_t slot_at, n_slots;       // joint_lists_build
  int32_t M;                      // pattern nodes
  int32_t no_rss;                 // a model without secondary structure: rule 8 alone, the band tables are not read
  double* X; size_t x_stride;
  double* vec;                    // log-space form: 5 S doubles per thread of a workgroup of the fused scan kernel
  double* profile;
  double* counts;
};

// ---- pair posteriors by motif node pair and the pair counts behind a stem logo (stem_rules.h, stem_kernels.hip).  A launch covers
// the G sequences idx[0 .. G) of one group or chunk; slot g of the launch owns the per-cell scratch X + g * x_stride: Q of every
// cell by stem slot (stem_at).  has[n] = 1 once batch index n has Q (a parse, and a model with secondary structure).  The counts
// of batch index n go to counts + 25 K * n at (k 5 + bl) 5 + br; its list entries to the staging range that starts at K * koff[n].
struct StemArgs {
  const SeqPlan* plans;           // batch plans (batch index)
  const int32_t* idx;             // idx[g] = batch index of the sequence in slot g (launch_stem_counts, launch_stem_seq)
  const double* seq_out; int32_t out_stride;   // row[4] != 0: the sequence left the double range (the log-space form covers it)
  int32_t skip_flagged;           // 1: leave the sequences flagged in seq_out alone (scaled-linear form)
  const uint8_t* seq;             // base codes of the batch (BatchArrays::seq)
  const uint32_t* okbits;         // the pair mask of the batch
  const int32_t* lists;           // the pair transitions by stem slot (stem_lists_build)
  int32_t K, n_list;              // stem slots, ints of the lists
  double* X; size_t x_stride;
  int32_t* has;
  double* counts;
  double min_prob;
  const int64_t* koff; int64_t* cnt;   // kept cells before batch index n (launch_pair_kept / launch_pair_prefix), entries staged
  int32_t* st_i; int32_t* st_j; uint8_t* st_k; double* st_q;   // staging (null: no list is kept)
};

// ---- helix posteriors (helix_rules.h, helix_kernels.hip).  A launch covers the G sequences idx[0 .. G) of one group or chunk; slot g
// of the launch owns one int of n_units, u_stride ints each of ui, ud and nlen, and max_len u_stride doubles of X: its units -- outer
// kept cells (ui, ud) in (i, d) order --, the lengths 1 .. nlen[r] unit r reached and their values (helix_at, rows of max_len).  The
// list entries of batch index n go to the staging range that starts at (max_len - min_len + 1) koff[n]; the stems of its caller-given
// structure are s_i / s_d / s_len[soff[n] .. soff[n + 1]) and their joint probabilities go to s_p.
struct HelixArgs {
  const SeqPlan* plans;           // batch plans (batch index)
  const int32_t* idx;             // idx[g] = batch index of the sequence in slot g (launch_helix_units, launch_helix_seq)
  const double* seq_out; int32_t out_stride;   // row[4] != 0: the sequence left the double range (the log-space form covers it)
  int32_t skip_flagged;           // 1: leave the sequences flagged in seq_out alone (scaled-linear form)
  const uint32_t* okbits;         // the pair mask of the batch
  int32_t max_len, min_len;
  int32_t no_rss;                 // a model without secondary structure: no units, the band tables are not read
  double min_prob;
  const double* P; size_t p_stride;   // scaled-linear form: P(i, d) of the slot ([i][d], rows of W+1; launch_pair_cells) picks the units
  int32_t* n_units; int32_t* ui; int32_t* ud; int32_t* nlen; size_t u_stride;
  double* X;
  double* vec;                    // log-space form: two state vectors per thread of a workgroup of the fused scan kernel
  const int64_t* koff; int64_t* cnt;   // kept cells before batch index n (launch_pair_kept / launch_pair_prefix), entries staged
  int32_t* st_i; int32_t* st_j; uint8_t* st_k; double* st_h;   // staging (null: no list is kept)
  const int64_t* soff; const int32_t* s_i; const int32_t* s_d; const int32_t* s_len; double* s_p;   // stems (soff null: none)
};

// ---- loop posteriors (loop_rules.h, loop_kernels.hip).  A launch covers the G sequences idx[0 .. G) of one group or chunk; slot g of
// the launch owns one int of n_units, u_stride ints each of ui and ud, 5 u_stride doubles of cols and t_stride doubles of T: its
// units -- outer kept cells (ui, ud) in (i, d) order, picked by k_helix_units from P --, the columns H S B I M of unit r at
// cols[5 r ..] and the two-loop values of the unit's items at their by-outer positions (the item's index in the plan of the
// sequence).  A closing entry of batch index n goes to the staging range that starts at koff[n] (6 doubles: p and the columns), a
// two-loop entry to the range that starts at the sequence's item_base (the item's index and T); counts + 5 n receives the column
// sums over the units; the loops of its caller-given structure are s_type / s_i / s_d / s_k / s_l[soff[n] .. soff[n + 1]) and their
// probabilities go to s_p.
struct LoopArgs {
  const SeqPlan* plans;           // batch plans (batch index)
  const int32_t* idx;             // idx[g] = batch index of the sequence in slot g (launch_loop_seq)
  const double* seq_out; int32_t out_stride;   // row[4] != 0: the sequence left the double range (the log-space form covers it)
  int32_t skip_flagged;           // 1: leave the sequences flagged in seq_out alone (scaled-linear form)
  const uint32_t* okbits;         // the pair mask of the batch
  int32_t no_rss;                 // a model without secondary structure: no units, the band tables are not read
  int32_t want_units;             // the lists or the counts are asked for: units are picked and walked
  double min_prob;                // the lists' threshold (+inf: no lists)
  double bound;                   // the units' threshold on P: loop_pick_bound(min_prob), 0 where the counts are asked for
  double* P; size_t p_stride;     // P(i, d) of the slot ([i][d], rows of W+1): launch_pair_cells, or the fused scan kernel
  int32_t* n_units; int32_t* ui; int32_t* ud; size_t u_stride;
  double* cols;
  double* T; size_t t_stride;
  const LoopItem* items; const int32_t* by_outer_off; const uint8_t* item_in;   // the plan's arrays (k_loop_seq, k_loop_scatter)
  double* counts;                 // null: not asked for
  const int64_t* koff; int64_t* cnt; int64_t* cnt2;   // kept cells before batch index n, closing / two-loop entries staged
  int32_t* st_i; int32_t* st_j; double* st_v;          // closing staging (null: no lists are kept)
  int32_t* st2_it; double* st2_t;                      // two-loop staging
  const int64_t* soff; const int32_t* s_type; const int32_t* s_i; const int32_t* s_d; const int32_t* s_k; const int32_t* s_l;
  double* s_p;                    // loops of the structures (soff null: none)
};
// the final lists of a loop call, as k_loop_scatter fills them: batch index n has cnt[n] closing entries from staging koff[n] on that
// go to off[n] .., and cnt2[n] two-loop entries from staging item_base on that go to off2[n] ..
struct LoopListCols {
  const SeqPlan* plans; const LoopItem* items;
  const int64_t* koff; const int64_t* cnt; const int64_t* off; const int64_t* cnt2; const int64_t* off2;
  const int32_t* st_i; const int32_t* st_j; const double* st_v; const int32_t* st2_it; const double* st2_t;
  int32_t* c_seq; int32_t* c_i; int32_t* c_j; double* c_v;                              // closing list, 6 doubles per entry
  int32_t* t_seq; int32_t* t_i; int32_t* t_j; int32_t* t_k; int32_t* t_l; double* t_p;  // two-loop list
};

// ---- maximum expected accuracy motif alignments and site lists (node_mea_rules.h, node_mea_kernels.hip) over the profile of the
// whole batch: batch index n with seq_base b and length L writes the row of slot k at node + max_sites * b + k * L (the sampler's
// layout), n_sites[n], and start / end / score / conf at [n * max_sites + k]
struct NodeMeaArgs {
  const SeqPlan* plans;           // batch plans (batch index)
  const int32_t* lists;           // lo, first, last per node (node_mea_lists_build)
  int32_t M, max_sites;
  double gamma;
  const double* profile;          // NodeArgs::profile of the same call
  uint8_t* bp;                    // scratch: M bytes per position of the batch, the predecessor of every (position, node)
  uint8_t* node; int32_t* n_sites; int32_t* start; int32_t* end; double* score; double* conf;
};

struct DpArgs {
  AutomatonLayout lay;            // host-visible copy (launch geometry, LDS sizes)
  const AutomatonLayout* layp;    // the same record in device memory: kernels read it through this pointer
  const int32_t* ints;     // automaton blob (global)
  const double* params;    // ParamBlock followed by theta[n_theta]
  int32_t no_prf, m_min, no_rss;
  int32_t first_pass_only;  // debug: TRAIN stops after the full-terminal outside pass
  int32_t cyk_only;         // SCAN: Ys / Ye are given in sc_ys / sc_ye (batch pipeline); run the Viterbi pass and traceback only
  const SeqPlan* plans;
  const int32_t* order;    // processing order (longest first)
  int32_t n_seq;
  int32_t* counter;        // work queue head
  BatchArrays b;
  const uint32_t* okbits;
  PlanArrays p;
  // table slots, one per workgroup
  double* band_in; double* band_out; double* ext_in; double* ext_out;
  size_t band_stride, ext_stride;  // in doubles
  double* tmp; size_t tmp_stride;  // heavy-sum temporaries: 3 * tmp_stride doubles per slot, tmp_stride = (Lmax+1)*S
  TraceRec* tr_ext;
  // TRAIN: per-sequence results [n][out_stride] = Zo, Zari, Znasi, f, skipped, bpp_eff, ENo[nt], ENx[nt], EHo[2], EHx[2]
  double* seq_out;
  int32_t out_stride;
  // BPP: filtered mask + efficiency
  uint32_t* okbits_out;
  double log_min_bpp;
  double* lnbpp_out;   // optional per-cell ln BPP (debug), indexed by cell_base
  // SCAN outputs (batch offsets: seq_base for start/inner/psihat/rss, pos_base for end)
  double* sc_start; double* sc_end; double* sc_inner; int32_t* sc_psihat; char* sc_rss;
  int32_t* sc_ys; int32_t* sc_ye; double* sc_exist; double* sc_en;  // sc_en: [n][n_theta]
  int32_t* trace_stack; int32_t trace_stack_stride;
  long long* prof;  // optional [n_blocks][8] cycle counters: stage, in-band, in-ext, out-ext, out-band, other
  LdsLayout lds;
  // SCAN, base-pair posteriors (pair_rules.h): non-null = stop after inside + the first outside pass and write P(i, d) of the
  // sequence order[w] to pair_p + w * pair_stride ([i][d], rows of W+1; 0 where the cell is not kept)
  double* pair_p; size_t pair_stride;
  // SCAN, samples (sample_rules.h, log-space form): n_samples > 0 = stop after the inside pass and draw the samples of sequence
  // order[w] on the slot's dense log tables, the workgroup's lanes over the samples
  SampleArgs smp;
  // SCAN, motif-conditional pair posteriors (cond_rules.h, log-space form): non-null = stop after inside + one outside pass per
  // world (terminals ari alone, then nasi alone) and write P_motif / P_none of the sequence order[w] to cond_p0 / cond_p1 +
  // w * pair_stride (as pair_p) and ln Z(ari, nasi), ln Z(ari), ln Z(nasi) to cond_z + 4 w
  double* cond_p0; double* cond_p1; double* cond_z;
  // SCAN, structural context profiles (ctx_rules.h, log-space form): ctx.u non-null = stop after inside + the first outside pass
  // and write P, u, h, b and o of the sequence order[w] to slot w of ctx (the rows k_ctx_seq reads behind the launch)
  CtxArgs ctx;
  // SCAN, posterior motif-node profiles (node_rules.h, log-space form): node.profile non-null = stop after inside + the first
  // outside pass and write the M columns of every position of the sequence order[w]
  NodeArgs node;
  // SCAN, accessibility (access_rules.h, log-space form): acc.T non-null = stop after inside + the first outside pass and write the
  // four planes of the sequence order[w] to slot w of acc (the rows k_access_seq reads behind the launch)
  AccessArgs acc;
  // SCAN, joint node-by-context posteriors (joint_rules.h, log-space form): jnt.profile non-null = stop after inside + the first
  // outside pass and write the 7 M columns of every position of the sequence order[w] (k_joint_counts reads them behind the launch)
  JointArgs jnt;
  // SCAN, pair posteriors by motif node pair (stem_rules.h, log-space form): stm.X non-null = stop after inside + the first outside
  // pass and write Q of the sequence order[w] to slot w of stm (k_stem_counts and k_stem_seq read it behind the launch)
  StemArgs stm;
  // SCAN, helix posteriors (helix_rules.h, log-space form): hlx.X non-null = stop after inside + the first outside pass and write the
  // units of the sequence order[w] -- every cell of its band, in (i, d) order -- to slot w of hlx (k_helix_seq reads them behind the
  // launch) and the probabilities of its stems to hlx.s_p
  HelixArgs hlx;
  // SCAN, loop posteriors (loop_rules.h, log-space form): lop.cols non-null = stop after inside + the first outside pass and write P,
  // the units of the sequence order[w] -- every cell of its band, in (i, d) order, the columns of a cell that is no unit 0 --, their
  // columns and two-loop values to slot w of lop (k_loop_seq reads them behind the launch) and the probabilities of the loops of its
  // structure to lop.s_p
  LoopArgs lop;
};

// arguments of the diagonal-synchronous train pipeline (train_kernels.hip)
struct TrArgs {
  AutomatonLayout lay;
  const AutomatonLayout* layp;
  const int32_t* ints;
  const double* params;
  int32_t no_prf, m_min, no_rss, first_pass_only;
  int32_t lik_ratio;    // --lik-ratio objective (ELEMDP_LIK_RATIO)
  int32_t schedule;     // 0 = the reference's two outside passes, 1 = ari-only + restricted nasi-only (linear)
  int32_t restricted;   // set per launch: this pass sweeps the one-state automaton
  const AutomatonLayout* layp_r; const int32_t* ints_r;
  const SeqPlan* plans;
  const int32_t* grp;   // grp[g] = batch index of the sequence in table slot g
  BatchArrays b;
  const uint32_t* okbits;
  PlanArrays p;
  double* band_in; double* band_out; double* ext_in; double* ext_out;
  size_t band_stride, ext_stride;
  double* tmp; size_t tmp_stride;
  double* seq_out; int32_t out_stride;
  int32_t pass, d;
};
struct BppOut {
  uint32_t* okbits_out;   // filtered pair mask (batch-level, bits_base indexing)
  int32_t* kept;          // kept pairs per sequence (index = position in the plan array)
  double* lnbpp;          // optional ln BPP per cell (cell_base indexing) or null
  double log_min_bpp;
};
// arguments of the linear-semiring BPP filter (bpp_kernels.hip): a chunk of sequences, `plans` = their records with
// cell_base / dmin_base counted from the start of the chunk (seq_base, bits_base: batch level)
// widest band whose Boltzmann weights stay inside the double range with a margin: a GC-rich helix of n stacked pairs weighs
// about e^(5.5 n) (3.4 kcal/mol per stack at kT = 0.616), and a span of W holds at most W / 2 of them -- e^550 at W = 200
// against the limit e^709; wider bands go through the log-space filter (k3_bpp_*)
constexpr int kBppLinMaxSpan = 200;
constexpr int kBppInPlanes = 7 + BC_CLASSES + 1, kBppOutPlanes = 5 + BC_CLASSES;
struct BppLinArgs {
  const EnergyTables* et;
  const EnergyTables* xet;         // the same tables exponentiated (exp_tables): interior loops through loop_weight
  const BppCandTable* cand;        // candidate table of the interior loops (null: the mask walk of round 2)
  int16_t* plist; int32_t* poff;   // pairs of every diagonal of a sequence, ascending ([cell_base + ..], [seq * poff_stride + d]); null: diagonal launches
  int32_t poff_stride, pmax;       // pmax = most canonical pairs of a sequence of the chunk
  int32_t lmax, wmax;              // set by launch_bpp_lin
  unsigned long long* prof;        // debug (ELEMDP_BPP_PROF): cycles of wave 0 of every workgroup per phase [direction][8], or null
  const SeqPlan* plans;
  const uint8_t* seq;
  const uint32_t* okbits;          // canonical pair mask
  int16_t* dmin;                   // [dmin_base + i]: smallest canonical span starting at i (0: none)
  double* xw; size_t xw_stride;    // exp of the five structural terms [term][cell_base + d * (L+1) + i]
  double* tin; double* tout; size_t t_stride;   // band tables [plane][cell_base + d * (L+1) + i]: kBppInPlanes inside / kBppOutPlanes outside planes
  double* lo_in; double* lo_out;   // exterior chains as logarithms [dmin_base + j]
  int32_t no_ene, min_span, m_min, d;
  uint32_t* okbits_out;            // filtered mask (bits_base indexing)
  int32_t* kept;                   // kept pairs per sequence of the chunk
  double* lnbpp;                   // optional ln BPP per candidate [cell_base + i * (W+1) + d], or null
  double log_min_bpp;
};
hipError_t launch_bpp_lin(const BppLinArgs& a, int G, int Lmax, int Wmax, hipStream_t st);
// arguments of the scaled-linear train pipeline (lin_kernels.hip, rules in lin_rules.h)
struct LinArgs {
  AutomatonLayout lay;            // automaton swept by this launch: the full one, or the compact one-state one (S = 1)
  const AutomatonLayout* layp;
  const int32_t* ints;
  const double* params;           // ParamBlock + log theta (lambda, lam_same)
  const double* lin;              // linear parameter block (lin_rules.h: tau, psb, log2 psb, eth)
  int32_t no_prf, m_min, no_rss;
  const SeqPlan* plans;
  const int32_t* grp;             // grp[g] = batch index of the sequence in table slot g
  const SeqPlan* plans_slot;      // the plans of this group in slot order (saves the grp -> plans dependent load), or null
  BatchArrays b;
  const double* ews;              // exp of the position weights
  const uint32_t* okbits;
  PlanArrays p;
  const double* xwc; size_t xwc_stride;   // exp(lambda_k * structural term): [k*5+term][cell]
  const double* xwi; size_t xwi_stride;   // exp(lambda_k * tsc) of the interior-loop items: [k][item]
  double* band_in; double* band_out; double* ext_in; double* ext_out;   // tables swept by this launch
  size_t band_stride, ext_stride;
  double* zs;                     // per slot: mantissas of Z(ari,nasi), Z(ari), Z(nasi), and log2 of the sequence's scale
  double* seq_out; int32_t out_stride;
  int32_t schedule, pass, d;
  int32_t cpb;                    // cells of one block = lanes of a workgroup / lanes per cell of the unary phase
  float rcp_nap, rcp_lane, rcp_cpb;   // 1 / n_ap, 1 / lanes per cell, 1 / cpb for the lane -> (cell, item) splits of the band
                                  // kernels (div_rcp: a reciprocal formed per lane costs ten instructions and a register for the whole kernel)
  int32_t* flagged;               // [0] = number of flagged sequences, [1..] = their batch indices
  // scan (sum passes K4 / K5 on this pipeline): start constraint and position-posterior accumulators (batch offsets)
  int32_t lik_ratio;              // --lik-ratio objective (ELEMDP_LIK_RATIO)
  int32_t scan;                   // 1: only Z(ari,nasi) decides the range check
  int32_t* ys; int32_t* ye;       // per batch index: argmax start / end
  double* pos_start; double* pos_inner; double* pos_end; double* exist;
  // scan, Viterbi pass on the batch pipeline: trace tables per slot (same indexing as the band / ext tables), outputs
  TraceRec* tr_ext; int32_t* sc_psihat; char* sc_rss; int32_t* trace_stack; int32_t trace_stack_stride;
  long long* prof;                // optional [16] shader-clock sums per phase (thread 0 of every workgroup), or null
  // rule 2, factorised (lin_rules.h): pair tables [d][i][p] per slot (a_stride doubles each) and the end-indexed pair mask
  // (bits_base indexing, like okbits)
  double* a_in; double* a_out; size_t a_stride;
  const uint32_t* okbits_end;
  int32_t lmax, nword_max;        // longest sequence of the launch / most pair-mask words of a sequence (LDS sizing)
  int32_t wmax;                   // largest span of the launch (sizes the position window staged in LDS)
  int32_t n_stage;                // ints of the automaton blob staged in LDS: n_ints (whole blob) or n_small
  int32_t dbg;                    // timing experiments only: bit 0 skip split sums, 1 skip item sums, 2 skip the unary phase
  int32_t ext_ring;               // exterior-chain kernels keep the chain's last rows in an LDS ring (small groups only)
  int32_t ext_block;              // steps of the inside exterior chain whose pair sums are formed side by side (4 where every pair
                                  // spans >= 5 positions -- the default mask --, else 1)
  int32_t n_lin;                  // doubles of the linear parameter block the band kernels stage (with or without the weight tables)
  int32_t fast;                   // train: table-driven unary phases (lin_fast.h); the host clears it where they do not apply
  int32_t det;                    // train: deterministic reductions -- every heavy sum of a workgroup gets its adds from ONE wave (pairs of
                                  // a cell in one wave: det_sh; tuples dealt to the waves by target: AutomatonLayout::qd_*), the
                                  // statistics one copy per wave, one row of counts per (sequence, block):
                                  // det_rows[n][det_nslot][out_stride], summed in order by k4_combine
  int32_t cyk_compact;            // scan, Viterbi pass: the table in the compact layout (TableView::ldm / stm), set by launch_cyk_group
  int32_t det_sh;                 // log2 of the lanes a cell's pairs take in the pair phases of the deterministic mode (a power of two
                                  // >= n_ap, so that no cell straddles two waves); -1: more than 64 pairs, one wave does the phase
  double* det_rows; int32_t det_nslot;
  // train sweeps from the live-block lists of the plan (p.blocks non-null): the cells a block may span (the window of positions a
  // workgroup stages; 0 without lists: cpb) and, for the launcher alone, the HOST array of the largest block count per diagonal
  // (negative: this diagonal keeps consecutive cells)
  int32_t live_span;
  const int32_t* blk_grid;
  // loop pre-pass (option loop_prepass; k4_in_loops): 1 = the inside sweep of the table-driven train form takes its L plane from
  // the pre-pass (the engine sets it where the mask is on and the automaton's loop states all have an L column); in_d0 = the first
  // diagonal with an entry outside the L plane (first_inside_diagonal); blk_grid_in = blk_grid of the inside set (p.blocks_in)
  int32_t loop_pre = 0, in_d0 = 0;
  const int32_t* blk_grid_in = nullptr;
  // the outside L plane behind the sweep (option loop_outside; k4_out_lrows): 1 = the outside sweep of the table-driven
  // train form computes and stores no L, takes the inside set of lists and starts no diagonal below in_d0 (the engine sets it where
  // loop_pre could be set and the mode is not the deterministic one)
  int32_t loop_post = 0;
  // scan, motif-conditional pair posteriors (cond_rules.h).  scan_terms: the terminals an outside sweep of the scan is seeded with
  // -- 0 = ari and nasi with Z(ari, nasi), 1 = ari alone with Z(ari), 2 = nasi alone with Z(nasi); a sequence whose world is empty
  // (Z = 0) is left alone by that sweep.  range_all: 1 = the range check of the inside pass looks at all three Z, as the train
  // evaluation's does, except that a Z of exactly 0 is an empty world and no range failure
  int32_t scan_terms = 0, range_all = 0;
  // scan family, option world: the world whose Z normalises the products behind launch_lin_world_group -- the index
  // into the slot's zs: 0 = Z(ari, nasi), 1 = Z(ari), 2 = Z(nasi)
  int32_t world = 0;
  // train sweeps under the mask: 1 = every entry the mask calls useless already holds its 0 in these slots (an earlier evaluation of
  // the same plan on the same slots stored it: TableSlots::zeros), so the sweeps store none -- no fill of dead cells or rows, no 0
  // from the dead branch of the pair phases, dead workgroups return at once
  int32_t zeros_kept = 0;
};
struct LinWeightArgs {
  const LoopItem* items_inner; const LoopItem* items_left; const LoopItem* items_right;   // (may be null)
  const double* e_stack; const double* e_ext; const double* e_ml; const double* e_close; const double* e_hp;
  const LoopItem* items;
  size_t n_cells, n_items;       // cells of the batch (= stride of the planes of xwc), items
  size_t cell_first = 0, cell_count = 0;   // cells to compute (count 0: all) -- an evaluation of a range of the batch
  const double* params;
  double* xwc; double* xwi;
};
hipError_t launch_lin_weights(const LinWeightArgs& a, hipStream_t st);
// one whole train evaluation of a group; `full` sweeps the pattern automaton, `compact` (schedule 1) the one-state
// automaton of the no-motif pass over the compact tables
// scan: SCAN_PASS_START = inside + outside with start / inner posteriors and argmax start; SCAN_PASS_END = the same constrained
// to that start with end posteriors and argmax end (RNAelemScanDP::operator(), motif_scanner.hpp:186-202); SCAN_PASS_INSIDE = the
// inside sweeps and the exterior chain of SCAN_PASS_START only (Z and the range check, no outside pass: the tables of the sampler,
// sample_rules.h)
// SCAN_PASS_OUT_ARI / SCAN_PASS_OUT_NASI = an outside sweep alone, behind SCAN_PASS_INSIDE on the same slots, seeded with the ari
// terminals / the nasi terminal only (LinArgs::scan_terms): the outside tables of one world of cond_rules.h, no pick
enum ScanPass { SCAN_PASS_START = 0, SCAN_PASS_END = 1, SCAN_PASS_INSIDE = 2, SCAN_PASS_OUT_ARI = 3, SCAN_PASS_OUT_NASI = 4 };
hipError_t launch_lin_scan_group(const LinArgs& full, int G, int Lmax, int Wmax, ScanPass pass, hipStream_t st);
// the tables a product of the scan family reads, in the world full.world: 0 = SCAN_PASS_START as it stands; 1 / 2 =
// SCAN_PASS_INSIDE, then k_world_empty (a sequence whose world is empty, Z_w = 0 exactly, is handed to the log-space form as a
// sequence without a parse is, so that no product kernel meets an outside row the sweep skipped), then SCAN_PASS_OUT_ARI / _NASI
hipError_t launch_lin_world_group(const LinArgs& full, int G, int Lmax, int Wmax, hipStream_t st);
// the argument record a product kernel of the scan family is launched with: zs moved to the world's Z, so that the kernel's
// zs[4 g] (LViews::zs[0]) is Z_w -- the product kernels are the same code in every world
inline LinArgs lin_in_world(const LinArgs& a) {
  LinArgs b = a;
  b.zs += a.world;
  return b;
}
// scan: Viterbi parse (max-plus CYK with trace records, then traceback) of a group; uses band_in / ext_in as the CYK table
hipError_t launch_cyk_group(const LinArgs& full, int G, int Lmax, int Wmax, hipStream_t st);
hipError_t launch_lin_group(const LinArgs& full, int G, int Lmax, int Wmax, bool first_pass_only, hipStream_t st);
hipError_t launch_bpp_group(const TrArgs& base, const BppOut& o, int G, int Lmax, int Wmax, hipStream_t st);
hipError_t launch_train_group(const TrArgs& base, int G, int Lmax, int Wmax, hipStream_t st);

hipError_t launch_mask(const BatchArrays& b, const SeqPlan* plans, int n_seq, int min_span, bool write_bits, uint32_t* okbits,
                       int32_t* n_canonical, hipStream_t st);
// constraint_kernels.hip: the pair mask of a constrained batch from the filter's mask `in` (it may be `okbits` itself: in place)
// and the per-position rows of constraint_derive (indexed like BatchArrays::unp, SeqPlan::pos_base)
hipError_t launch_constrain(const SeqPlan* plans, int n_seq, int nword_max, const uint8_t* cls, const int32_t* partner,
                            const int32_t* enc, const uint32_t* in, uint32_t* okbits, hipStream_t st);
hipError_t launch_plan_cells(const PlanKernelArgs& a, int32_t* n_items_out, hipStream_t st);
hipError_t launch_plan_items(const PlanKernelArgs& a, hipStream_t st);
hipError_t launch_useful_mask(const PlanKernelArgs& a, size_t n_cells, size_t lds_cap, hipStream_t st);   // needs dmin (launch_plan_cells)
void useful_mask_host(const uint8_t* kept, const uint8_t* unp, int L, int W, int C, int m_min, bool no_ene, uint8_t* out);
bool useful_mask_fits(const PlanKernelArgs& a, size_t lds_cap);   // false: launch_useful_mask stores the mask of all ones
// the pair-term words of every sequence of the set from its finished mask (a.p.useful -> a.p.ha_rows, a.p.h1_stems); wmax1 <= 65
hipError_t launch_pair_terms(const PlanKernelArgs& a, hipStream_t st);
// the same words on the host from a mask[(W+1)*(L+1)] and the kept pairs kept[(L+1)*(W+1)] of one sequence, W <= 64
void pair_terms_host(const uint8_t* mask, const uint8_t* kept, int L, int W, unsigned long long* ha, unsigned long long* h1);
// the live-block lists of every sequence of the set from its mask (a.p.useful -> a.p.blocks of n_records records, a.blk_max),
// cells per block a.live_cpb;
// with a.p.blocks_in non-null also the inside set; a.blk_max holds 6 rows of wmax1 ints either way
hipError_t launch_live_blocks(const PlanKernelArgs& a, size_t n_records, hipStream_t st);
// the same lists on the host from a mask [d][i] of (W+1) * (L+1) bytes: counts[d] blocks of diagonal d at records + d * stride
// (stride >= ceil((L + 1) / cpb) records of 16 bytes)
// (bits: the planes that make a cell live, live_blocks.h)
void live_blocks_host(const uint8_t* mask, int L, int W, int cpb, int cap, int32_t* counts, LiveBlock* records, int stride, int bits = 0xff);
// can the loop pre-pass serve the automaton of this host blob?  (the L rows fit the pre-pass's staging, and a loop state without an
// L column has the L value 0 in the sweep's own rule too; min_span: the smallest span of a kept pair)
bool lin_loop_prepass_ok(const AutomatonLayout& lay, const int32_t* ints, int min_span);
// ... and the L kernels behind the outside sweep (option loop_outside), on top of lin_loop_prepass_ok
bool lin_loop_outside_ok(const AutomatonLayout& lay, const int32_t* ints);
// cells per block of the table-driven train sweeps of these arguments, 0 where they run another form (no lists then); the
// largest span a block's live cells may cover in this build
int lin_train_cpb(const LinArgs& full);
int lin_live_span_max();
hipError_t launch_plan_sort(const PlanKernelArgs& a, hipStream_t st);   // the sort of launch_plan_items alone (sort_roles = 0 before)
hipError_t launch_permute_items(const PlanKernelArgs& a, hipStream_t st);
bool plan_copies_fused(const PlanKernelArgs& a);   // launch_plan_items has written the item copies already (no launch_permute_items)
hipError_t launch_dp(int kind, const DpArgs& a, int n_blocks, hipStream_t st);
hipError_t launch_reduce(const double* seq_out, int out_stride, int n_seq, int n_theta, double* partial, hipStream_t st);
const char* dp_kernel_name(int kind);

// ---- base-pair posteriors (pair_rules.h, pair_kernels.hip).  A launch covers the G sequences idx[0 .. G) of one group or chunk;
// slot g of the launch owns P + g * p_stride ([i][d], rows of W+1).
struct PairArgs {
  const SeqPlan* plans;           // batch plans (batch index)
  const int32_t* idx;             // idx[g] = batch index of the sequence in slot g
  const uint32_t* okbits;         // pair mask after the filter (bits_base indexing)
  // launch_pair_cells: the compact tables of the group's slots, P plane (AutomatonLayout::tab_*): rows start at
  // tab_cs[P] * cells + (d * (L+1) + i) * p_rs; the real states' columns are 0 .. ncol-1
  const double* band_in; const double* band_out; size_t band_stride;
  int32_t p_cs, p_rs, ncol;
  const double* zs;               // per slot: the Z mantissa that normalises P at zs[4 g] (LinArgs::zs + LinArgs::world)
  const double* seq_out; int32_t out_stride;   // row[4] != 0: the sequence left the double range (the log-space form covers it)
  int32_t skip_flagged;           // 1: leave the sequences flagged in seq_out alone (scaled-linear form)
  double* P; size_t p_stride;
  // launch_pair_seq
  double min_prob;
  double* unpaired;               // seq_base indexing, L values per sequence
  const int64_t* koff;            // per batch index: first staging entry (prefix of the kept pairs)
  int32_t* st_i; int32_t* st_j; double* st_p;   // staging list, (i, j) in row order per sequence
  int64_t* cnt;                   // per batch index: pairs with P >= min_prob
  // launch_pair_mea (mea_rules.h): w = RN(mea_gamma2 * P), mea_gamma2 = 2 gamma; slot g owns mea_M + g * p_stride ([i][d], as P)
  // and mea_ch + g * mea_ch_stride (the choices of M, then those of the exterior chain); the structure at seq_base, the score at n
  double mea_gamma2;
  double* mea_M; int32_t* mea_ch; size_t mea_ch_stride;
  char* mea_s; double* mea_score;
};
hipError_t launch_pair_cells(const PairArgs& a, int G, int cells_max, hipStream_t st);   // k4_pairs
hipError_t launch_pair_seq(const PairArgs& a, int G, hipStream_t st);
// k_pair_mea, behind launch_pair_seq on the same slots and stream; Wmax >= the W of every sequence of the launch (LDS size)
hipError_t launch_pair_mea(const PairArgs& a, int G, int Wmax, hipStream_t st);

// ---- motif-conditional pair posteriors (cond_rules.h, cond_kernels.hip).  A launch covers the G sequences idx[0 .. G) of one group
// or chunk; slot g of the launch owns P[w] + g * p_stride ([i][d], rows of W+1) for the worlds w = 0 (motif) and 1 (none).
struct CondArgs {
  const SeqPlan* plans;           // batch plans (batch index)
  const int32_t* idx;             // idx[g] = batch index of the sequence in slot g
  const uint32_t* okbits;         // pair mask after the filter (bits_base indexing)
  // launch_cond_cells: the P plane of the group's compact table slots, as PairArgs
  const double* band_in; const double* band_out; size_t band_stride;
  int32_t p_cs, p_rs, ncol;
  // per slot: Z(ari, nasi), Z(ari), Z(nasi) at z[4 g ..] -- mantissas in the tables' scale (z_log 0), or logarithms (z_log 1)
  const double* z; int32_t z_log;
  const double* seq_out; int32_t out_stride;   // row[4] != 0: the sequence left the double range (the log-space form covers it)
  int32_t skip_flagged;           // 1: leave the sequences flagged in seq_out alone (scaled-linear form)
  double* P[2]; size_t p_stride;
  // launch_cond_seq
  double min_prob;
  double* unpaired[2];            // seq_base indexing, L values per sequence
  double* exist; double* shift;   // per batch index
  const int64_t* koff;            // per batch index: first staging entry (prefix of the kept pairs)
  int32_t* st_i; int32_t* st_j; double* st_p[2];   // staging list, (i, j) in row order per sequence
  int64_t* cnt;                   // per batch index: pairs with max(P_motif, P_none) >= min_prob
};
// k4_cond behind launch_lin_scan_group (SCAN_PASS_OUT_ARI: world 0, SCAN_PASS_OUT_NASI: world 1) on the same slots and stream
hipError_t launch_cond_cells(const CondArgs& a, int world, int G, int cells_max, hipStream_t st);
// k_cond_seq behind both worlds' reductions, or behind the fused scan kernel (DpArgs::cond_p0)
hipError_t launch_cond_seq(const CondArgs& a, int G, hipStream_t st);
// (the final list, ordered by (sequence, i, j) with two probability columns: launch_list_scatter)

hipError_t launch_sample(const LinArgs& a, const SampleArgs& s, int G, hipStream_t st);
// k_ctx_cells behind launch_lin_scan_group (SCAN_PASS_START) and launch_pair_cells on the same slots and stream; k_ctx_seq behind
// it, or behind the fused scan kernel (DpArgs::ctx)
hipError_t launch_ctx_cells(const LinArgs& a, const CtxArgs& c, int G, int cells_max, hipStream_t st);
hipError_t launch_ctx_seq(const CtxArgs& c, int G, hipStream_t st);
// k_access_chains behind launch_lin_scan_group (SCAN_PASS_START) on the same slots and stream (n_vec: the entries of a state vector,
// max(S, n_ap); Lmax: the longest sequence of the group); k_access_seq behind it, or behind the fused scan kernel (DpArgs::acc)
hipError_t launch_access_chains(const LinArgs& a, const AccessArgs& c, int G, int Lmax, int n_vec, hipStream_t st);
hipError_t launch_access_seq(const AccessArgs& c, int G, hipStream_t st);
// k_node_pos behind launch_lin_scan_group (SCAN_PASS_START) on the same slots and stream: one wave per (sequence, position)
hipError_t launch_node_pos(const LinArgs& a, const NodeArgs& c, int G, int Lmax, hipStream_t st);
// k_joint_rows (one wave per row of a sequence: the hairpin and bulge chains, per-cell sums by node) and k_joint_pos (one wave per
// (sequence, position): the 7 M columns) behind launch_lin_scan_group (SCAN_PASS_START) on the same slots and stream;
// k_joint_counts behind them, or behind the fused scan kernel (DpArgs::jnt)
hipError_t launch_joint_rows(const LinArgs& a, const JointArgs& c, int G, int Lmax, hipStream_t st);
hipError_t launch_joint_pos(const LinArgs& a, const JointArgs& c, int G, int Lmax, hipStream_t st);
hipError_t launch_joint_counts(const JointArgs& c, int G, hipStream_t st);
// k_stem_cells (one lane per cell: Q by stem slot) behind launch_lin_scan_group (SCAN_PASS_START) on the same slots and stream;
// k_stem_counts (one workgroup per sequence: the K 25 counts) and k_stem_seq (its list entries with q >= min_prob into its staging
// range) behind it, or behind the fused scan kernel (DpArgs::stm); launch_list_scatter: the batch list in (sequence, i, j, slot) order
hipError_t launch_stem_cells(const LinArgs& a, const StemArgs& c, int G, int cells_max, hipStream_t st);
hipError_t launch_stem_counts(const StemArgs& c, int G, int Lmax, int Wmax, hipStream_t st);
hipError_t launch_stem_seq(const StemArgs& c, int G, hipStream_t st);

// ---- helix posteriors (helix_kernels.hip), behind launch_lin_scan_group (SCAN_PASS_START) and launch_pair_cells on the same slots
// and stream: k_helix_units (one workgroup per sequence: the kept cells whose P reaches min_prob, in (i, d) order), k_helix_chains
// (one wave per unit or stem: the chain of helix_rules.h); k_helix_seq (one workgroup per sequence: its list entries in (i, j, len)
// order into its staging range) behind them, or behind the fused scan kernel (DpArgs::hlx); launch_list_scatter: the batch list
hipError_t launch_helix_units(const HelixArgs& c, int G, hipStream_t st);
hipError_t launch_helix_chains(const LinArgs& a, const HelixArgs& c, int G, int cells_max, hipStream_t st);
hipError_t launch_helix_seq(const HelixArgs& c, int G, hipStream_t st);

// ---- loop posteriors (loop_kernels.hip), behind launch_lin_scan_group (SCAN_PASS_START), launch_pair_cells and launch_helix_units
// (the units: the compaction scheme is shared) on the same slots and stream: k_loop_unary (one lane per unit: H, S, M), k_loop_items
// (one wave per unit: the two-loop values of its items, B and I), k_loop_struct (one lane per loop of the caller-given structure);
// k_loop_seq (one workgroup per sequence: the counts, and its entries of both lists into its staging ranges) behind them, or behind
// the fused scan kernel (DpArgs::lop); launch_loop_scatter: the batch lists
hipError_t launch_loop_unary(const LinArgs& a, const LoopArgs& c, int G, int cells_max, hipStream_t st);
hipError_t launch_loop_items(const LinArgs& a, const LoopArgs& c, int G, int cells_max, hipStream_t st);
hipError_t launch_loop_struct(const LinArgs& a, const LoopArgs& c, int G, int Lmax, hipStream_t st);
hipError_t launch_loop_seq(const LoopArgs& c, int G, hipStream_t st);
hipError_t launch_loop_scatter(const LoopListCols& c, int n, hipStream_t st);
// k_node_mea behind the node pass of the whole batch (both forms), on the engine's stream: one wave per sequence
hipError_t launch_node_mea(const NodeMeaArgs& a, int n_seq, hipStream_t st);
// ---- the staged lists of the pair, conditional, stem and helix calls (staged_list.h, pair_kernels.hip).  The columns of one list, as
// k_list_scatter takes them: batch index n has cnt[n] entries in staging from mult * koff[n] on, and its entries of the final list
// start at off[n].  A null st_v[1] or st_k: the list has no second value column, or no label column.
struct ListCols {
  const int64_t* koff; const int64_t* cnt; const int64_t* off;
  int64_t mult;                   // staging entries per kept cell (1; the stem slots K; the lengths of the helix list)
  const int32_t* st_i; const int32_t* st_j; const double* st_v[2]; const uint8_t* st_k;
  int32_t* seq; int32_t* i; int32_t* j; double* v[2]; int32_t* k;   // final list: seq = n, the label widened to int32
};
// kept pairs of every sequence of the batch (the staging capacity), off[0..n] = exclusive prefix of cnt[0..n) with off[n] the total,
// and the scatter of the staging list into the final list ordered by (sequence, i, j[, label])
hipError_t launch_pair_kept(const SeqPlan* plans, const uint32_t* okbits, int n, int64_t* kept, hipStream_t st);
hipError_t launch_pair_prefix(const int64_t* cnt, int n, int64_t* off, hipStream_t st);
hipError_t launch_list_scatter(const ListCols& c, int n, hipStream_t st);

}  // namespace elemdp
