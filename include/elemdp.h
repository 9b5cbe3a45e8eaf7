/* elemdp.h -- C ABI of libelemdp.so, the MI355X-native inside/outside/CYK engine.
 *
 * The reference (iyak/RNAelem @ 2024_08_07) has no FFI: its de-facto operator interface for this
 * path is C++ duck typing,
 *     int  RNAelemTrainer::operator()(V const& x, double& fn, V& gr)   RNAelem/motif_trainer.hpp:595
 *     void RNAelemScanner::scan(RNAelem& model)                        RNAelem/motif_scanner.hpp:938
 * consumed by Lbfgsb::minimize / Adam::minimize (RNAelem/optimizer.hpp:146, :298) and main()
 * (RNAelem/main.cpp:47-130).  This header is the boundary a maintainer would bind instead
 * (INTEGRATION.md shows the C++ shim that drops into motif_trainer.hpp / motif_scanner.hpp).
 *
 * Conventions: plain pointers and sizes only; every function returns 0 on success, a negative
 * ELEMDP_E* code otherwise (elemdp_last_error() gives the message); no exceptions cross the
 * boundary.  Caller owns every buffer it passes; inputs are copied during the call.  One handle =
 * one GPU = one caller thread.  The library has NO CPU fallback: without a usable HIP device
 * elemdp_create fails with ELEMDP_ENODEV.
 */
#ifndef ELEMDP_H
#define ELEMDP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define ELEMDP_ABI_VERSION 1

enum { /* status codes */
  ELEMDP_OK = 0,
  ELEMDP_EINVAL = -1,  /* bad argument / malformed pattern or parameter text */
  ELEMDP_ENODEV = -2,  /* no HIP device */
  ELEMDP_EHIP = -3,    /* HIP runtime error */
  ELEMDP_ESTATE = -4,  /* call order (e.g. train_eval before load_batch) */
  ELEMDP_ENOMEM = -5,
};

enum { /* elemdp_model_desc.flags */
  ELEMDP_NO_RSS = 1 << 0,        /* --no-rss       RNAelem/application.hpp:259, motif_model.hpp:171-206 */
  ELEMDP_NO_PROFILE = 1 << 1,    /* --no-profile   RNAelem/application.hpp:265 */
  ELEMDP_NO_ENERGY = 1 << 2,     /* --no-energy    RNAelem/application.hpp:271 */
  ELEMDP_THETA_SOFTMAX = 1 << 3, /* --theta-softmax RNAelem/application.hpp:289 */
  ELEMDP_LIK_RATIO = 1 << 4,     /* --lik-ratio: a sequence without motif contributes Z(ari) - Z(ari,nasi) and the statistics of
                                    those two terminal sets (RNAelem/motif_trainer.hpp:156-202, --no-shuffle branch) */
  /* runtime forms of the reference's compile-time test switches (RNAelem/const_options.hpp:12-24) */
  ELEMDP_DBG_FIX_RSS = 1 << 9,   /* structure fixed per sequence (elemdp_load_batch `fix_rss`) */
  ELEMDP_DBG_NO_TURN = 1 << 10,  /* hairpins of any size */
};

/* Model description == what main.cpp:89-101 / RNAelemReader::read_model (motif_io.hpp:118-262)
 * put into an `RNAelem` object before the optimizer / scanner is started. */
typedef struct {
  const char* pattern;      /* search pattern, e.g. "((.*.))"         --motif-pattern        */
  const char* energy_param; /* ViennaRNA-2.0 parameter TEXT, or NULL / "~T2004~" / "~A2007~"
                               for the shipped tables (data dir: elemdp_set_data_dir)      */
  int32_t max_span;         /* --max-span           (default 50)                            */
  int32_t max_iloop;        /* --max-internal-loop  (default 30)                            */
  double min_bpp;           /* --min-bpp            (default 1e-4; 0 = no BPP filter)       */
  double tau;               /* --tau                (default 0.1)                           */
  int32_t flags;            /* ELEMDP_* bits                                                */
  int32_t device;           /* HIP device ordinal; -1 = current                             */
} elemdp_model_desc;

typedef struct elemdp_handle elemdp_handle;

const char* elemdp_last_error(void);
int elemdp_abi_version(void);
/* directory holding turner2004.elempar / andronescu2007.elempar (default: next to the library) */
int elemdp_set_data_dir(const char* dir);

/* Builds the pattern automaton (RNAelem::set_motif_pattern, motif_model.hpp:80-97) and the energy
 * tables (EnergyModel::set_param_file, energy_model.hpp:153-161), uploads them, creates streams. */
int elemdp_create(const elemdp_model_desc* desc, elemdp_handle** out);
int elemdp_destroy(elemdp_handle* h);

/* Sizes: n_param = #theta entries + 2 (pack_params order, motif_model.hpp:147-157);
 * n_state = S interval states; n_node = M pattern nodes (incl. 'z' and 'o'). */
int elemdp_n_param(const elemdp_handle* h);
int elemdp_n_state(const elemdp_handle* h);
int elemdp_n_node(const elemdp_handle* h);
/* x0 exactly as the reference CLI builds it: uniform log-probability rows (profile_hmm.hpp:286-313;
 * zeros when theta-softmax), then lambda_init twice (motif_trainer.hpp:565). */
int elemdp_initial_params(const elemdp_handle* h, double lambda_init, double* x, int32_t n_param);
/* JSON description of the automaton (states, transition lists) for inspection / host-logic tests. */
int elemdp_describe(const elemdp_handle* h, char* buf, int32_t cap);

/* Engine knobs (not part of the reference interface).  Unknown keys are ELEMDP_EINVAL.
 *   evaluation
 *     "pipeline"        4 (default): scaled-linear batch pipeline, which hands sequences outside the double range to the log-space
 *                       one; 3: log-space batch pipeline for everything.  (2, the fused kernel of round 1, is retired.)
 *     "schedule"        1 (default): ONE outside sweep for both passes of motif_trainer.hpp:209-225 -- "has motif" terminals on
 *                       the pattern's states, "no motif" terminal on a shadow copy of state (0,0); 0: the reference's two sweeps
 *     "fast"            1 (default): table-driven band kernels (per-state programs, weight tables, cell records); 0: generic rule code
 *     "deterministic"   1: bit-identical repeats of elemdp_train_eval (fixed summation order, as the reference at --thread 1); slower
 *     "eval_first", "eval_count"   a train evaluation covers the records [first, first + count) of the resident batch only
 *                       (count 0 = all; reset by elemdp_load_batch).  Refused (ELEMDP_EINVAL) for a streamed batch and for pipeline 3
 *     "prune"           1 (default): transition lists without what cannot occur in a complete parse; 0: the reference's complete lists
 *     "first_pass_only" debug: stop a train evaluation after the first outside pass
 *   batches
 *     "max_resident"    most sequences kept resident at a time (0 = as many as the device memory holds): a larger batch is STREAMED --
 *                       elemdp_train_eval / elemdp_scan run it in chunks of that size, the BPP filter + plan of chunk k+1 built on a
 *                       second inner engine and host thread while chunk k is evaluated, partial sums added in chunk order; set
 *                       before elemdp_load_batch
 *     "group"           sequences swept in lockstep (0 = as many as fit); "group_streams": groups evaluated concurrently (default 2);
 *                       "slots": table slots; "two_streams": retired with pipeline 2, accepted and ignored
 *     "keep_lnbpp"      keep ln BPP of the filter for elemdp_batch_pairs; "bpp_log": 1 = log-space BPP filter for every band
 *     "sorted_plan"     1: role lists of the plan sorted per cell (reproducible summation order of the log-space pipeline)
 *     "live_blocks"     1 (default): a workgroup of the train sweeps takes its cells from the plan's lists of LIVE cells (non-zero
 *                       mask byte) of the diagonal instead of consecutive ones (elemdp_live_blocks) on the diagonals where that leaves fewer workgroups;
 *                       2: on every diagonal; 0: consecutive cells.  Needs
 *                       "useful_mask"; the deterministic mode keeps consecutive cells whatever the value;
 *     "live_span"       the cells the live cells of one block may span, up to 64 (a model with more cells per block than
 *                       the value takes its cells per block); 0 (default): 32;
 *     "useful_mask"     1 (default): the train sweeps skip the table entries no complete parse reaches (elemdp_useful_mask);
 *                       0: they compute every entry -- kept as the A/B switch and as the tests' reference
 *     "pair_terms"      1 (default): the pair sums of the outside train sweep (rule 2, factorised) walk the plan's words
 *                       (elemdp_pair_terms): HA takes its work items from the useful parent rows of its stem cells instead of
 *                       every row up to the span, H1 walks the useful stems of its cell instead of every kept pair that starts
 *                       at the cell's end -- the dropped terms are exact zeros that were never added; ignored where the plan
 *                       has no words (a span above 64, the mask of all ones, "useful_mask" 0) and in the deterministic mode;
 *                       0: every row and stem -- the A/B switch and the tests' reference
 *     "loop_prepass"    1 (default): a row pre-pass fills the inside L plane before the table-driven train sweep, whose workgroups
 *                       then compute no L, skip the cells that are useful in the L plane alone (lists of their own:
 *                       elemdp_live_blocks_inside) and the diagonals below the first hairpin; active wherever "useful_mask" is,
 *                       the deterministic mode included (every L entry is bit-identical to the sweep's own); 0: the sweep
 *                       computes L itself, with one set of lists -- the A/B switch and the tests' reference
 *     "loop_outside"    1 (default): the outside L plane -- the rule-6c sums of the loops, the chain L <- L, the 6b energy statistic
 *                       and the right-emission counts of the chain -- is made by two kernels behind the table-driven outside
 *                       sweep, which then computes no L, sums the item records of the inner pairs alone, and takes the lists
 *                       of elemdp_live_blocks_inside (built for it where "loop_prepass" is 0); active wherever "useful_mask" is,
 *                       except in the deterministic mode, where it is ignored; 0: the sweep computes L itself -- the A/B
 *                       switch and the tests' reference
 *     "own_slots"       1 (default): an unranged train evaluation of a resident batch gives every sequence a table slot of its
 *                       own where the batch fits the sizing rules (about twice the table memory of the bench configuration);
 *                       the zeros of the entries "useful_mask" calls useless then stay in the slots from one evaluation to the
 *                       next of the same plan and options, and are not stored again (elemdp_last_timing entries 3 and 4 say
 *                       whether, and how many slots the handle holds); 0: the slots of one group, shared by the groups of a
 *                       stream.  The sequences swept in lockstep and the streams are the same either way
 *   the ensemble of the posterior products
 *     "world"           0 (default): the mixture every scan-family call describes, terminals ari and nasi, Z(ari, nasi) -- the
 *                       parses with the motif and those without it in the proportion exist_prob : 1 - exist_prob; 1: the parses
 *                       with the motif alone (terminals ari, Z(ari)); 2: the parses without it alone (terminal nasi, Z(nasi)); any
 *                       other value is ELEMDP_EINVAL.  In world w every product is its own rule on the inside tables of the first
 *                       sum pass, which the worlds share, and the outside tables of a sweep seeded with world w's terminals alone,
 *                       normalised with Z_w: elemdp_pair_posteriors in world 1 / 2 is the P_motif / P_none of
 *                       elemdp_pair_conditional.  Honoured by elemdp_pair_posteriors and elemdp_pair_mea (with elemdp_pair_list),
 *                       elemdp_sample (the terminal is drawn among the world's terminals alone, draw 0 is consumed as ever, logp is
 *                       relative to Z_w), elemdp_context_profile, elemdp_node_profile, elemdp_node_mea, elemdp_joint_profile,
 *                       elemdp_stem_profile (with elemdp_stem_list), elemdp_helix_posteriors (with elemdp_helix_list),
 *                       elemdp_loop_posteriors (with its two lists and the loops and stems of caller-given structures) and
 *                       elemdp_accessibility.  Ignored by elemdp_scan (its record is the reference's), by
 *                       elemdp_pair_conditional (both worlds by definition) and by the train calls.  A world with Z_w = 0
 *                       exactly is empty: the call returns for that sequence what it returns for a sequence without any parse --
 *                       P = 0 and unpaired 1, no list entries, structure all '.', context O = 1, profile 1 at node 0 (J(p, 0, O)
 *                       = 1), counts 0, no sites, accessibility 1, sample status 1 (no parse) -- through the same path, the
 *                       log-space form (elemdp_last_timing entry 2 counts the sequence); no outside sweep runs for it.  Setting
 *                       the option keeps the cached masks of a streamed batch and, set again, replaces its entry in the record
 *                       of options the inner engines of a streamed batch replay (elemdp_last_timing entry 5: the number of
 *                       entries)
 *   measurement / tests
 *     "profile"         in-kernel phase clocks for elemdp_debug_profile; "dbg": switch phases off (results invalid);
 *     "poison"          1: every table is filled with NaN before an evaluation (an unmasked read of an entry nobody stored shows) */
int elemdp_set_option(elemdp_handle* h, const char* key, double value);

/* Replaces the resident batch (== FastqReader contents, fastq_io.hpp:64-108):
 *   seq_codes : concatenated base codes N,A,C,G,U -> 0..4 (bio_sequence.hpp:28-39)
 *   seq_off   : n_seq+1 offsets;   qual : char-33 values, L+1 per sequence;   qual_off likewise
 *   fix_rss   : NULL, or concatenated dot-bracket strings (seq_off indexing) with ELEMDP_DBG_FIX_RSS
 * Runs the parameter-independent part once on the GPU and keeps it resident:
 * the BPP filter (EnergyModel::set_seq .. fill_bpp_tables, energy_model.hpp:211-276) and the
 * structural energy terms of every admissible rule (energy_param.hpp:686-795). */
int elemdp_load_batch(elemdp_handle* h, const uint8_t* seq_codes, const int32_t* seq_off, const uint8_t* qual,
                      const int32_t* qual_off, const char* fix_rss, int32_t n_seq);
/* elemdp_load_batch with a hard structure constraint per sequence:
 *   constraint : NULL (then the call is elemdp_load_batch(..., NULL, ...)), or the concatenated constraint strings in seq_off
 *                indexing, one character per base:  . free   x unpaired   | paired   < paired, 5' base   > paired, 3' base
 *                ( ) these two bases pair with each other (balanced, nested; a canonical pair within the span limits)
 * The BPP filter runs unconstrained (elemdp_batch_bpp_eff is the filter's); behind it the pair mask keeps the filter's pairs the
 * strings allow plus the forced pairs, and every later call -- train, scan, every posterior -- describes the constrained
 * ensemble.  A string no structure satisfies is no error: the sequence has no parse.  ELEMDP_EINVAL: an unknown character, an
 * unbalanced string, a forced pair that is not canonical (the message names sequence and bases), or a handle made with
 * ELEMDP_DBG_FIX_RSS or ELEMDP_NO_RSS. */
int elemdp_load_batch_constrained(elemdp_handle* h, const uint8_t* seq_codes, const int32_t* seq_off, const uint8_t* qual,
                                  const int32_t* qual_off, const char* constraint, int32_t n_seq);
/* Host only: the same mask rule on the CPU for one sequence of L bases (codes in seq), W = min(L, max_span), from the filter's
 * pairs kept[(L+1)*(W+1)] (as elemdp_batch_pairs gives them) and a 0-terminated string of L characters: kept_out (same shape)
 * and unp_out[L+1], "position may be emitted unpaired".  flags: ELEMDP_DBG_NO_TURN is looked at. */
int elemdp_constraint_mask_host(const uint8_t* kept, const uint8_t* seq, const char* constraint, int32_t L, int32_t W,
                                int32_t flags, uint8_t* kept_out, uint8_t* unp_out);
/* per-sequence results of the BPP filter: bpp_eff[n_seq] (energy_model.hpp:265) */
int elemdp_batch_bpp_eff(elemdp_handle* h, double* bpp_eff, int32_t n_seq);
/* kept[(L+1)*(W+1)] (index i*(W+1)+d) of one sequence after the filter; lnbpp may be NULL */
int elemdp_batch_pairs(elemdp_handle* h, int32_t seq_index, uint8_t* kept, double* lnbpp, int32_t cap);
/* Debug: the usefulness mask of one sequence of the resident plan, mask[(W+1)*(L+1)] (index d*(L+1)+i, like the tables).  Bits:
 * 1 P, 2 E, 4 M, 8 B, 16 A (pair entries of the factorised rule 2), 32 plane 1, 64 plane 2, 128 L -- set where a complete parse
 * can pass through the entry with every weight taken as positive (a superset of that set). */
int elemdp_useful_mask(elemdp_handle* h, int32_t seq_index, uint8_t* mask, int32_t cap);
/* Host only: the same mask by the same rules on the CPU from the kept pairs of one sequence, kept[(L+1)*(W+1)] (index
 * i*(W+1)+d, as elemdp_batch_pairs gives them); W = min(L, max_span); unp: L flags "may be unpaired" or NULL (all may);
 * flags: ELEMDP_NO_ENERGY and ELEMDP_DBG_NO_TURN are looked at. */
int elemdp_useful_mask_host(const uint8_t* kept, const uint8_t* unp, int32_t L, int32_t W, int32_t max_iloop, int32_t flags,
                            uint8_t* mask);
/* Debug: the live-block lists of one sequence of the resident plan for the cells per block of the model and the span of the
 * current options (built by the call if no evaluation has built them): counts[d], d = 0 .. W, blocks of
 * diagonal d in records + 16 * (d * stride + b).  A record is 16 bytes: uint64 live (bit k: cell first + k is live), int16 first,
 * int16 own_lo, int16 own_end (the block owns the cells [own_lo, own_end)), int16 count.  stride >= (L + 8) / 8.  cpb_cap[2]
 * receives the cells per block and the span a block may cover.  taken[W+1] (may be NULL) receives 1 where a train evaluation of
 * the current options ("live_blocks", "useful_mask", "deterministic") sweeps diagonal d from
 * its list, 0 where it takes consecutive cells -- the outside sweep, and the inside sweep without the loop pre-pass; behind the
 * pre-pass ("loop_prepass" 1) the inside sweep takes the second set, elemdp_live_blocks_inside. */
int elemdp_live_blocks(elemdp_handle* h, int32_t seq_index, int32_t* counts, void* records, int32_t stride, int32_t* cpb_cap,
                       int32_t* taken);
/* Host only: the same lists by the same rule on the CPU from a mask[(W+1)*(L+1)] (any non-zero byte is a live cell) for blocks
 * of cpb live cells that span at most cap cells, cpb <= cap <= 64 (else ELEMDP_EINVAL); stride >= ceil((L + 1) / cpb). */
int elemdp_live_blocks_host(const uint8_t* mask, int32_t L, int32_t W, int32_t cpb, int32_t cap, int32_t* counts, void* records,
                            int32_t stride);
/* Debug: as elemdp_live_blocks, for the second set of lists of the plan -- the lists of the inside sweep behind the loop pre-pass
 * (option "loop_prepass"), in which a cell is live where its mask byte has a bit other than 128 (L).  taken[d] = 1 where a train
 * evaluation of the current options sweeps diagonal d of the inside pass from this list: never without the pre-pass, and never on
 * a diagonal below the first one that can hold an entry outside the L plane (no inside launch there at all). */
int elemdp_live_blocks_inside(elemdp_handle* h, int32_t seq_index, int32_t* counts, void* records, int32_t stride, int32_t* cpb_cap,
                              int32_t* taken);
/* Host only: elemdp_live_blocks_host with the bits that make a cell live (1 .. 255; 255 = any non-zero byte, 127 = the inside set). */
int elemdp_live_blocks_host_bits(const uint8_t* mask, int32_t L, int32_t W, int32_t cpb, int32_t cap, int32_t bits, int32_t* counts,
                                 void* records, int32_t stride);
/* Debug: the pair-term words of one sequence of the resident plan (built with the mask by the call if no
 * evaluation has built them), (W+1)*(L+1) words each, index d*(L+1)+i like the mask.  ha_rows: bit b-1 of the word of a kept pair
 * (i, d) is set where the term outA(i-b, i+d) x 1(i-b, i) of its HA sum can be non-zero; h1_stems: bit sp-1 of the word of cell
 * (i, d) where the term outA(i, j+sp) x P(j, j+sp), j = i+d, of its H1 sum can.  Both hold the same triples.  Fails where the plan
 * has no words: a span above 64, or the mask of all ones. */
int elemdp_pair_terms(elemdp_handle* h, int32_t seq_index, uint64_t* ha_rows, uint64_t* h1_stems, int32_t cap);
/* Host only: the same words by the same rules on the CPU from a mask[(W+1)*(L+1)] and the kept pairs kept[(L+1)*(W+1)] of one
 * sequence (as elemdp_useful_mask_host takes them); W <= 64 (else ELEMDP_EINVAL). */
int elemdp_pair_terms_host(const uint8_t* mask, const uint8_t* kept, int32_t L, int32_t W, uint64_t* ha_rows, uint64_t* h1_stems);

/* == RNAelemTrainer::operator()(x, fn, gr) over the whole resident batch with --no-shuffle
 * (motif_trainer.hpp:595-633 + RNAelemTrainDP::operator() :124-272).  fn/gr are the UNREGULARISED
 * sums (the optimizer adds rho*x^2/2, optimizer.hpp:246-260).  sum_eff = sum of bpp_eff over used
 * sequences (:227); n_skipped = sequences with non-finite Z (:211-215). */
int elemdp_train_eval(elemdp_handle* h, const double* x, int32_t n_param, double* fn, double* gr,
                      double* sum_eff, int32_t* n_skipped);

/* Multi-GPU form: the same evaluation, but stops before the cross-rank sum.  `partial` (device or
 * host pointer, elemdp_partial_len(h) doubles) receives this rank's
 *   [fn, sum_eff, n_used, n_skipped, ENo[n_theta], ENx[n_theta], EHo[2], EHx[2]]
 * The caller all-reduces (sum) it over RCCL -- the MI355X replacement of the reference's
 * file-based array-job sum (motif_array_trainer.hpp:20-58) -- and then calls
 * elemdp_train_finish on the reduced vector (host pointer) to obtain fn / gr. */
int elemdp_partial_len(const elemdp_handle* h);
int elemdp_train_partial(elemdp_handle* h, const double* x, int32_t n_param, void* partial, int32_t partial_is_device);
int elemdp_train_finish(elemdp_handle* h, const double* reduced, double* fn, double* gr, double* sum_eff,
                        int32_t* n_skipped);
/* Host-only: tells the handle which x a following elemdp_train_finish refers to (needed for the
 * softmax chain rule, motif_trainer.hpp:251-261) when elemdp_train_partial ran in another handle. */
int elemdp_set_finish_params(elemdp_handle* h, const double* x, int32_t n_param);

/* In-library collective for hosts without their own (the reference binary with INTEGRATION.md's shim): one process (or
 * thread) per GPU, one handle each.  Rank 0 obtains an id with elemdp_comm_unique_id (128 bytes, ncclUniqueId) and hands
 * it to the other ranks by whatever means the host has (a file, MPI, a socket); every rank then calls elemdp_comm_init on
 * its handle.  From then on elemdp_train_eval all-reduces (sum, fp64, elemdp_partial_len doubles) the partial vector over
 * RCCL / xGMI on the engine's stream before it finishes fn / gr, so every rank returns the values of the WHOLE batch --
 * the replacement of the array job + result files of motif_array_trainer.hpp:20-58 (submit_array_job / collect_fn_gr_eff).
 * A rank whose share of the batch is empty calls elemdp_train_eval without a batch: it contributes zeros.
 * librccl.so is loaded on the first call (dlopen); without it these return ELEMDP_ENODEV. */
#define ELEMDP_COMM_ID_BYTES 128
int elemdp_comm_unique_id(void* id_out);
int elemdp_comm_init(elemdp_handle* h, int32_t rank, int32_t world, const void* id);
int elemdp_comm_destroy(elemdp_handle* h);

/* per-sequence diagnostics of the last train evaluation: 5 doubles per sequence
 * [Z(ari,nasi), Z(ari), Z(nasi), f_n, skipped] (motif_trainer.hpp:108-112, 204-227) */
int elemdp_train_seq_stats(elemdp_handle* h, double* out, int32_t n_seq);
/* per-sequence expected counts of the last train evaluation: 2 * n_theta + 4 doubles per sequence
 * [ENo[n_theta], ENx[n_theta], EHo[2], EHx[2]] (the terms of the reference's gradient, motif_trainer.hpp:229-249); all 0
 * for a skipped sequence, and for the sequences outside a ranged evaluation whatever the evaluation before left.  A resident
 * batch only: ELEMDP_ESTATE while the handle streams its batch, before any train evaluation of the loaded batch, and after
 * a scan-family call (which writes rows of its own). */
int elemdp_train_seq_counts(elemdp_handle* h, double* out, int32_t n_seq);
/* debug: tables of ONE sequence after a train evaluation of a batch holding only that sequence:
 * inside_o/outside_o [(L+1)*S]; inside/outside [(L+1)*(W+1)*7*S] in the reference's index order
 * [i][d][e][s] (motif_trainer.hpp:62-65); outside = the first (full-terminal) pass.  Any may be NULL.
 * ENo/ENx [n_theta], EH [4] = EHo,EHx.  ELEMDP_ESTATE before any train evaluation of the loaded batch and, as
 * elemdp_train_seq_counts, after a scan-family call (whose tables are not a train evaluation's). */
int elemdp_debug_tables(elemdp_handle* h, double* inside, double* outside, double* inside_o, double* outside_o,
                        double* ENo, double* ENx, double* EH);

/* == RNAelemScanner::scan (motif_scanner.hpp:938-949, per-sequence worker :215-260), input order
 * preserved.  Caller-provided arrays use the batch offsets: start/inner at seq_off[n] (L values),
 * end at qual_off[n] (L+1 values), psihat/rss at seq_off[n]; per-sequence scalars indexed by n. */
typedef struct {
  double* start;      /* log P(motif starts at p)                  "start:"  */
  double* end;        /* log P(motif ends at p | start = Ys)       "end:"    */
  double* inner;      /* log P(p inside motif)                     "inner:"  */
  int32_t* psihat;    /* CYK motif node per position               "psihat:" */
  char* rss;          /* CYK structure letters O L R H B I M       "rss:"    */
  int32_t* ys;        /* argmax start (last maximum, util.hpp:232) "motif region:" */
  int32_t* ye;
  double* exist_prob; /* exp(logsumexp(start))                     "exist prob:" */
  double* en;         /* n_theta expected emission counts summed over the batch ("E[N]:"), may be NULL */
} elemdp_scan_out;
int elemdp_scan(elemdp_handle* h, const double* x, int32_t n_param, elemdp_scan_out* out);

/* Base-pair probabilities of the resident batch under the motif model x: for every kept pair (i, j = i + d) of the BPP filter,
 * P(i, j) = sum over the interval states s of inside(i, j, P, s) * outside(i, j, P, s) / Z(ari, nasi) over the tables of the
 * scan's first sum pass (the motif-model counterpart of EnergyModel::lnBPP, energy_model.hpp:195-201, over
 * motif_scanner.hpp:186-192); bases i and j-1 (0-based) pair.  Keeps on the device the pairs with P >= min_prob (min_prob >= 0;
 * 0 = every kept pair) in (sequence, i, j) order and returns their number in *n_pairs; unpaired: NULL or seq_off indexing
 * (L values per sequence), unpaired(p) = 1 - the P of the pairs base p takes part in.  elemdp_last_timing afterwards:
 * [whole call, sum passes + pair kernels, sequences handed to the log-space form]. */
int elemdp_pair_posteriors(elemdp_handle* h, const double* x, int32_t n_param, double min_prob,
                           int64_t* n_pairs, double* unpaired);
/* elemdp_pair_posteriors (the same list for elemdp_pair_list, the same unpaired and elemdp_last_timing) and, over the same P, the
 * maximum expected accuracy structure of every sequence: with w(i, j) = 2 gamma P(i, j), the nested structure of
 * kept pairs, spans <= max_span, that maximises the sum of w over its pairs plus the sum of unpaired over its unpaired bases.
 * structure: NULL or seq_off indexing, L bytes '(' ')' '.' per sequence (no terminator); score: NULL or one value per sequence.
 * gamma must be finite and > 0 (else ELEMDP_EINVAL); min_prob = +inf keeps no list. */
int elemdp_pair_mea(elemdp_handle* h, const double* x, int32_t n_param, double min_prob, double gamma, int64_t* n_pairs,
                    double* unpaired, char* structure, double* score);
/* Stochastic samples of whole derivations of the motif x energy grammar: n_samples (> 0, else ELEMDP_EINVAL) draws
 * per sequence, each a structure together with its motif alignment, with its exact probability under the model.  The draws are a
 * pure function of (seed, batch index + index_base, sample index, draw index): a sharded or chunked run that passes the batch
 * offset of its first sequence as index_base draws what one whole run draws.  Sample k of a sequence with seq_off offset b and
 * length L: rss + n_samples * b + k * L, L structure letters O L R H B I M (as elemdp_scan's rss); node, at the same offset, L motif
 * nodes (psihat, one byte each: a model with more than 255 nodes is ELEMDP_EINVAL); logp[seq * n_samples + k], the log of the
 * derivation's probability.  status[seq]: 0 sampled, 1 no parse (Z = 0), 2 refused (a walk found no candidate with a positive
 * weight or exceeded its stack bound; that sample has blank letters, node 0 and a NaN log-probability, the others stay).  Sequences
 * that leave the double range of the scaled-linear tables, and every sequence under option pipeline 3, are sampled on the
 * log-space tables of the fused scan kernel.  Any output may be NULL.  elemdp_last_timing afterwards: [whole call, the same,
 * sequences handed to the log-space form].  elemdp_scan, the pair calls and the train calls are unaffected. */
int elemdp_sample(elemdp_handle* h, const double* x, int32_t n_param, int32_t n_samples, uint64_t seed, int64_t index_base,
                  char* rss, uint8_t* node, double* logp, int32_t* status);
/* Copies the list of the last elemdp_pair_posteriors / elemdp_pair_mea: seq (batch index), i, j (cell, j = i + d), p; any may be NULL.
 * cap < n_pairs is ELEMDP_EINVAL; before any elemdp_pair_posteriors (of the resident batch) ELEMDP_ESTATE. */
int elemdp_pair_list(elemdp_handle* h, int32_t* seq, int32_t* i, int32_t* j, double* p, int64_t cap);
/* Motif-conditional pair posteriors of the resident batch under the motif model x: the ensemble of
 * elemdp_pair_posteriors is a mixture of the parses with the motif (terminals ari) and those without it (terminal nasi); this call
 * gives the fold of each world on its own.  For every kept pair (i, j = i + d) of the BPP filter,
 *   P_motif(i, j) = sum_s inside(i, j, P, s) * outside_ari (i, j, P, s) / Z(ari)
 *   P_none (i, j) = sum_s inside(i, j, P, s) * outside_nasi(i, j, P, s) / Z(nasi)
 * with the outside tables of one outside sweep per world, seeded with that world's terminals alone, over one inside sweep.
 * Keeps on the device the pairs with max(P_motif, P_none) >= min_prob (min_prob >= 0; 0 = every kept pair; +inf keeps no list)
 * in (sequence, i, j) order and returns their number in *n_pairs.  exist_prob: one value per sequence, Z(ari) / Z(ari, nasi).
 * unpaired_motif, unpaired_none: seq_off indexing (L values per sequence), 1 - the world's P of the pairs base p takes part in.
 * structure_motif, structure_none: seq_off indexing, L bytes '(' ')' '.' per sequence (no terminator), the maximum expected
 * accuracy structure of elemdp_pair_mea over the world's P and unpaired; gamma is looked at only when one of them is given and
 * must then be finite and > 0 (else ELEMDP_EINVAL).  shift: one value per sequence, the sum over the kept pairs of
 * |P_motif - P_none| -- the expected number of base pairs that differ between the two folds, counted on marginals.  A world
 * without any parse (Z = 0) is empty: P = 0, unpaired = 1, structure all '.', shift NaN, and exist_prob 0 (no parse with the
 * motif, or none at all) or 1 (none without it).  Under ELEMDP_NO_RSS there are no pairs: empty list, unpaired 1, shift 0.
 * Sequences for which one of Z(ari, nasi), Z(ari), Z(nasi) is non-zero and leaves the double range of the scaled-linear tables,
 * and every sequence under option pipeline 3, go through the fused scan kernel in log space.  Any output but n_pairs may be
 * NULL.  elemdp_last_timing afterwards: [whole call, sweeps + reductions + decodes, sequences handed to the log-space form].
 * elemdp_scan, the pair, sample and profile calls (the list of the last elemdp_pair_posteriors included) and the train calls
 * are unaffected. */
int elemdp_pair_conditional(elemdp_handle* h, const double* x, int32_t n_param, double min_prob, double gamma,
                            int64_t* n_pairs, double* exist_prob, double* unpaired_motif, double* unpaired_none,
                            char* structure_motif, char* structure_none, double* shift);
/* Copies the list of the last elemdp_pair_conditional: seq (batch index), i, j (cell, j = i + d), p_motif, p_none; any may be
 * NULL.  cap < n_pairs is ELEMDP_EINVAL; before any elemdp_pair_conditional (of the resident batch) ELEMDP_ESTATE. */
int elemdp_pair_conditional_list(elemdp_handle* h, int32_t* seq, int32_t* i, int32_t* j, double* p_motif, double* p_none,
                                 int64_t cap);
/* Structural context profile of every position under the motif model x: profile[7 * (seq_off[n] + p) + c] is the
 * probability that base p (0-based) of sequence n has the rss letter c of "OLRHBIM" -- exterior, left or right base of a pair,
 * unpaired in a hairpin, bulge, interior or multi-branch loop -- over the ensemble of the scan's first sum pass (terminals ari and
 * nasi: the ensemble of elemdp_pair_posteriors, elemdp_pair_mea and elemdp_sample), from its inside / outside tables and Z(ari, nasi):
 *   L(p) = sum_d P(p, d), R(p) = sum_i P(i, p+1-i), P the pair posterior of elemdp_pair_posteriors;
 *   U(p) = sum_{i <= p} sum_s in(L, i, p+1, s) out(L, i, p+1, s) / Z: p is unpaired in a run of loop bases below a pair;
 *   H(p) = the posterior of rule 6b (hairpin), summed over the runs [i, j) that hold p;
 *   B(p) = the posterior of the rule-6c items of the inside pass with exactly one empty side, summed over the runs that hold p;
 *   I(p) = max(0, U - H - B);   O(p) = the posterior of rule 8 (exterior emission) at p;   M(p) = max(0, 1 - L - R - U - O).
 * The two remainders make a row sum to 1; they are exact wherever the tables' inside and outside agree.  With max_iloop < 30 the
 * reference's outside pass enumerates interior loops its inside pass does not: the tables carry that, elemdp_pair_posteriors
 * inherits it and so does this profile (U, hence I and M), which is why the remainders are clamped at 0.  A sequence without any
 * parse (Z = 0) has O = 1 and 0 elsewhere, exactly (unpaired = 1 of the pair call); under ELEMDP_NO_RSS every position has O = 1.
 * Sequences that leave the double range of the scaled-linear tables, and every sequence under option pipeline 3, go through the
 * same rule on the log-space tables of the fused scan kernel.  profile NULL is ELEMDP_EINVAL, a call before elemdp_load_batch
 * ELEMDP_ESTATE.  A row sums to 1 within 1e-12 for a sequence in the scaled-linear form; in the log-space form a term is
 * exp(a + b - ln Z), whose exponent rounds at eps |ln Z|, and the sum holds to about 1e-15 |ln Z| per term (within 1e-10 at
 * |ln Z| of a few thousand).  elemdp_last_timing afterwards: [whole call including the copy of the profile to the host, sum
 * passes + context kernels, sequences handed to the log-space form].  elemdp_scan, the pair calls (the list of the last one stays valid), elemdp_sample and the train calls are unaffected. */
int elemdp_context_profile(elemdp_handle* h, const double* x, int32_t n_param, double* profile);
/* Posterior motif-node profile of every position under the motif model x: with M = elemdp_n_node,
 * profile[M * (seq_off[n] + p) + m] is the probability that base p (0-based) of sequence n is emitted by pattern node m -- 0 is
 * 'z', M-1 is 'o', the numbering of psihat and of the node bytes of elemdp_sample -- over the ensemble of the scan's first sum pass
 * (terminals ari and nasi: the ensemble of elemdp_pair_posteriors, elemdp_sample and elemdp_context_profile), from its inside /
 * outside tables and Z(ari, nasi).  Every base of a derivation is emitted once, by one of five rules, and the profile is the sum of
 * their posteriors routed to the emitted node, clamped to [0, 1]:
 *   L <- L  in(L, i, d, s) out(L, i, d, s): node r(s) at j-1;      3a  out(2, i, d, s) wr in(2, i, d-1, s1): node r(s) at j-1;
 *   5a  out(M, i, d, s) wl in(M, i+1, d-1, sl): node l(sl) at i;   8   out_o(p+1, s) wt in_o(p, s1): node r(s) at p;
 *   1a / 1b  out(P, i, d, s) wp (in(P, i+1, d-2, sp) xst + in(E, i+1, d-2, sp)): node l(sp) at i and node r(s) at j-1.
 * There is no remainder column and no renormalisation: a row sums to 1 wherever the tables' inside and outside agree (within
 * 1e-12 for a sequence in the scaled-linear form, about 1e-15 |ln Z| per term in the log-space form); with max_iloop < 30 the
 * reference's outside pass enumerates interior loops its inside pass does not, and the sum follows the tables.  The sum over the
 * nodes 1 .. M-2 is exp(inner) of elemdp_scan.  A sequence without any parse (Z = 0) has profile 1 at node 0 and 0 elsewhere,
 * exactly; under ELEMDP_NO_RSS rule 8 alone carries the alignment.  Sequences that leave the double range of the scaled-linear
 * tables, and every sequence under option pipeline 3, go through the same rule on the log-space tables of the fused scan kernel.
 * profile NULL or more than 255 pattern nodes is ELEMDP_EINVAL, a call before elemdp_load_batch ELEMDP_ESTATE.
 * elemdp_last_timing afterwards: [whole call including the copy of the profile to the host, sum passes + node kernels, sequences
 * handed to the log-space form].  elemdp_scan, the pair calls (the list of the last one stays valid), elemdp_sample,
 * elemdp_context_profile and the train calls are unaffected. */
int elemdp_node_profile(elemdp_handle* h, const double* x, int32_t n_param, double* profile);
/* Joint node-by-context posteriors under the motif model x and the emission counts behind a motif logo.  With
 * M = elemdp_n_node and the letters c = O L R H B I M (the column order of elemdp_context_profile), J(p, m, c) is the probability
 * that base p of a sequence is emitted by pattern node m AND carries structure letter c, over the ensemble of the scan's first sum
 * pass (terminals ari and nasi, Z(ari, nasi): the ensemble of elemdp_context_profile and elemdp_node_profile), from its inside /
 * outside tables.  O, L, R and M are the rule-8, pair-left, pair-right and 3a + 5a parts of elemdp_node_profile routed by letter;
 * the L <- L part splits into H, B and I: the outside L entry is linear in its seeds, so the hairpin seeds (rule 6b) and the bulge
 * seeds (the rule-6c items with one empty run) are carried down every row by the L <- L chain on their own, and
 * I = max(0, L <- L part - H - B).  Every entry is clamped to [0, 1]; nothing is renormalised.  sum_c J(p, m, c) is the node
 * profile and sum_m J(p, m, c) the context profile, wherever the tables' inside and outside agree (max_iloop 30).
 *   counts:  required; counts[((n M + m) 7 + c) 5 + b] = sum_p J(p, m, c) [seq_n[p] = b], b = 0 .. 4 (N A C G U), reduced on
 *            the device in a fixed order: the logo table of a set of sequences is the sum of their blocks;
 *   profile: NULL, or 7 M doubles per position at 7 M (seq_off[n] + p) + 7 m + c (then the profile is copied to the host, else it
 *            stays on the device).
 * A sequence without any parse (Z = 0) has J(p, 0, O) = 1 and 0 elsewhere, exactly; under ELEMDP_NO_RSS rule 8 alone exists.
 * Sequences that leave the double range of the scaled-linear tables, and every sequence under option pipeline 3, go through the
 * same rule on the log-space tables of the fused scan kernel.  counts NULL or more than 255 pattern nodes is ELEMDP_EINVAL, a call
 * before elemdp_load_batch ELEMDP_ESTATE.  elemdp_last_timing afterwards: [whole call, sum passes + joint kernels, sequences handed
 * to the log-space form].  The other calls of the handle are unaffected; the list of the last pair call stays valid. */
int elemdp_joint_profile(elemdp_handle* h, const double* x, int32_t n_param, double* counts, double* profile);
/* Pair posteriors by motif node pair under the motif model x and the pair counts behind a stem logo.  The model
 * emits the two bases of a motif pair jointly: a pair transition s -> sp of the automaton emits the left base by node st_l(sp) and
 * the right base by node st_r(s).  A stem slot is a distinct node pair (left, right) over these transitions, slots in increasing
 * (left, right) order, K of them; elemdp_stem_slots writes the two node indices of every slot (both arrays NULL: only counts them)
 * and returns K.  It needs no device; cap < K is ELEMDP_EINVAL.  For a kept cell (i, j) and a slot k, Q(i, j, k) is the
 * probability that bases i and j-1 pair AND the pair is emitted by a transition of slot k, over the ensemble of the scan's first sum
 * pass (terminals ari and nasi, Z(ari, nasi): the ensemble of elemdp_pair_posteriors), from its inside / outside tables: the
 * rule-1a and rule-1b terms of elemdp_node_profile routed to the pair of nodes.  Every entry is clamped to [0, 1]; nothing is
 * renormalised.  sum_k Q(i, j, k) is the P of elemdp_pair_posteriors; summed over the slots of one left (right) node it is the L (R)
 * column of elemdp_joint_profile.
 *   counts:    required; counts[((n K + k) 5 + bl) 5 + br] = sum over the kept cells of Q(i, j, k) [seq_n[i] = bl] [seq_n[j-1] = br],
 *              base codes 0 .. 4 (N A C G U), reduced on the device in a fixed order: the stem table of a set of sequences is the
 *              sum of their blocks;
 *   min_prob:  >= 0, or +inf.  Finite: the entries (sequence, i, j, slot, q) with q = Q(i, j, k) >= min_prob are kept on the device
 *              in (sequence, i, j, slot) order for elemdp_stem_list, i 0-based and j exclusive as in elemdp_pair_list; at 0 the
 *              list holds every slot of every kept cell.  +inf: no list, and no staging is allocated;
 *   n_entries: NULL, or receives the length of the list.
 * A sequence without any parse (Z = 0) has counts 0 and no entries, exactly; so has every sequence under ELEMDP_NO_RSS, where the
 * band tables are not read.  Sequences that leave the double range of the scaled-linear tables, and every sequence under option
 * pipeline 3, go through the same rule on the log-space tables of the fused scan kernel.  counts or x NULL, min_prob negative or NaN,
 * more than 255 slots or pattern nodes: ELEMDP_EINVAL; a call before elemdp_load_batch: ELEMDP_ESTATE; elemdp_stem_list before any
 * stem call on the resident batch: ELEMDP_ESTATE, with cap below the length of the list: ELEMDP_EINVAL (its arrays may be NULL).
 * elemdp_last_timing afterwards: [whole call, sum passes + stem kernels, sequences handed to the log-space form].  The other calls
 * of the handle are unaffected; the lists of the last pair call and the last conditional call stay valid. */
int elemdp_stem_slots(const elemdp_handle* h, int32_t* node_left, int32_t* node_right, int32_t cap);
int elemdp_stem_profile(elemdp_handle* h, const double* x, int32_t n_param, double min_prob, double* counts, int64_t* n_entries);
int elemdp_stem_list(elemdp_handle* h, int32_t* seq, int32_t* i, int32_t* j, int32_t* slot, double* q, int64_t cap);
/* Helix posteriors under the motif model x.  Cells as in elemdp_pair_list: cell (i, j) pairs the 0-based bases i and
 * j-1.  The helix (i, j, len), len >= 1, is the event that the cells (i + t, j - t), t = 0 .. len-1, are all pairs: a run of len
 * directly stacked pairs whose outermost pair is (i, j).  H(i, j, len) is its probability over the ensemble of the scan's first sum
 * pass (terminals ari and nasi, Z(ari, nasi): the ensemble of elemdp_pair_posteriors), exact from its inside / outside tables: a
 * len-step path sum along the stacking rule (helix_rules.h), clamped to [0, 1], nothing renormalised.  H(i, j, 1) is the P of
 * elemdp_pair_posteriors, H is non-increasing in len, and H(i, j, len) <= H(i+1, j-1, len-1), wherever the tables' inside and outside
 * agree.  The pair marginals only bound it from above.
 *   max_len:   1 .. ELEMDP_HELIX_MAX_LEN; min_len: 1 .. max_len;
 *   min_prob:  >= 0, or +inf.  Finite: the entries (sequence, i, j, len, H) with min_len <= len <= max_len and H >= min_prob are kept
 *              on the device in (sequence, i, j, len) order for elemdp_helix_list; at 0 the list holds every (kept cell, len) whose
 *              len cells are all kept.  +inf: no list, and no staging is allocated;
 *   n_entries: NULL, or receives the length of the list;
 *   structure: NULL, or dot-bracket strings in seq_off indexing (L bytes per sequence, ( ) . only).  A stem is a maximal run of
 *              directly nested pairs of that structure.  stem_len and stem_prob (seq_off indexing; one of them may be NULL) receive,
 *              at the position of the 5' base of a stem's outermost pair, the stem's length -- not bounded by max_len -- and the joint
 *              probability of the whole stem; elsewhere 0 and NaN.  A stem that holds a pair that is not a kept cell, or a span above
 *              max_span, has probability 0 exactly.
 * A sequence without any parse (Z = 0) has no entries and stem probabilities 0, exactly; so has every sequence under ELEMDP_NO_RSS,
 * where the band tables are not read.  Sequences that leave the double range of the scaled-linear tables, and every sequence under
 * option pipeline 3, go through the same rule on the log-space tables of the fused scan kernel.  x NULL, max_len outside
 * 1 .. ELEMDP_HELIX_MAX_LEN, min_len outside 1 .. max_len, min_prob negative or NaN, an unbalanced structure or one with other
 * characters, a structure with both outputs NULL: ELEMDP_EINVAL; a call before elemdp_load_batch: ELEMDP_ESTATE; elemdp_helix_list
 * before any helix call on the resident batch: ELEMDP_ESTATE, with cap below the length of the list: ELEMDP_EINVAL (its arrays may
 * be NULL); no device: ELEMDP_ENODEV.  elemdp_last_timing afterwards: [whole call, sum passes + helix kernels, sequences handed to
 * the log-space form].  The other calls of the handle are unaffected; the lists of the last pair, conditional and stem call stay
 * valid, and a pair, conditional or stem call leaves the helix list alone. */
#define ELEMDP_HELIX_MAX_LEN 32
int elemdp_helix_posteriors(elemdp_handle* h, const double* x, int32_t n_param, int32_t max_len, int32_t min_len,
                            double min_prob, int64_t* n_entries,
                            const char* structure, int32_t* stem_len, double* stem_prob);
int elemdp_helix_list(elemdp_handle* h, int32_t* seq, int32_t* i, int32_t* j, int32_t* len, double* p, int64_t cap);
/* Loop posteriors under the motif model x: what every pair closes, and the two-loops.  Cells as in elemdp_pair_list:
 * cell (i, j) pairs the 0-based bases i and j-1.  Over the ensemble of the scan's first sum pass (terminals ari and nasi,
 * Z(ari, nasi): the ensemble of elemdp_pair_posteriors), exact from its inside / outside tables (loop_rules.h), every value clamped to
 * [0, 1], nothing renormalised.  For a kept cell the five columns, in the order of ELEMDP_LOOP_H .. ELEMDP_LOOP_M: the probability
 * that the pair closes a hairpin (H), stacks on the pair (i+1, j-1) (S), closes a bulge (B: one inner pair, one empty side), an
 * interior loop (I: one inner pair, bases on both sides) or a multi-branch loop (M).  M is the probability of the closing event
 * alone, whatever the shape of the loop: the joint probability of one particular multi-loop with all its branches is not formed.  The
 * two-loop (i, j, k, l) is the event that the pair (i, j) lies directly around the pair (k, l) with at least one unpaired base
 * between them; T is its probability; B and I are the sums of T over the two-loops of the cell.  H + S + B + I + M is the P of
 * elemdp_pair_posteriors and T <= P wherever the tables' inside and outside agree.
 *   min_prob:  >= 0, or +inf.  Finite: two lists are kept on the device.  The closing list (elemdp_loop_closing_list) holds the kept
 *              cells whose P reaches min_prob, in (sequence, i, j) order, with p = P and the five columns (cols: 5 doubles per
 *              entry): the membership rule and the order of elemdp_pair_list, applied to the P plane this call computes with the
 *              pair call's own reduction.  A call sweeps the tables anew and two sweeps agree to rounding, not bit for bit (two
 *              elemdp_pair_posteriors calls on one handle differ by a few 1e-16): against the list of a separate pair call at the
 *              same min_prob the cells and their order are the same and p agrees to rounding, except that a cell whose P lies
 *              within rounding of min_prob may be in one list only.  The two-loop list
 *              (elemdp_loop_two_list) holds every two-loop with T >= min_prob, ordered by its outer cell in (sequence, i, j) order
 *              and within an outer cell in the order of the plan's interior-loop items of that cell; at 0 it holds every two-loop
 *              of the inside enumeration whose two cells are kept.  An outer cell whose P lies in the rounding margin below
 *              min_prob (see counts) may have a two-loop listed without a closing entry.  +inf: no lists, and no staging is
 *              allocated;
 *   counts:    NULL, or 5 doubles per sequence: the expected number of loops of each type, the column sums over every kept cell
 *              whatever min_prob is, reduced on the device in a fixed order.  Their total is the expected number of pairs.  With
 *              counts every kept cell is walked; without, an outer cell whose P is below min_prob (less a relative margin of 2^-30
 *              for rounding) is not: T <= P, so no entry is lost;
 *   n_closing, n_two: NULL, or receive the lengths of the two lists;
 *   structure: NULL, or dot-bracket strings in seq_off indexing (L bytes per sequence, ( ) . only).  loop_type and loop_prob
 *              (seq_off indexing; one of them may be NULL) receive, at the position of the 5' base of every pair of the structure,
 *              the type of the loop that pair closes there (ELEMDP_LOOP_H .. ELEMDP_LOOP_M) and the probability of that loop --
 *              the column of the closing cell for H, S and M, the T of the two-loop for B and I --, with no threshold; elsewhere 0
 *              and NaN.  A pair that is not a kept cell (a span above max_span among them) gives 0 exactly, and so does a two-loop
 *              that is no item of the inside enumeration.  A B or I value is bit-equal to the entry of the two-loop list of the
 *              same call.
 * A sequence without any parse (Z = 0) has empty lists, counts 0 and loop probabilities 0, exactly; so has every sequence under
 * ELEMDP_NO_RSS, where the band tables are not read.  Sequences that leave the double range of the scaled-linear tables, and every
 * sequence under option pipeline 3, go through the same rule on the log-space tables of the fused scan kernel.  x NULL, min_prob
 * negative or NaN, an unbalanced structure or one with other characters, a structure with both outputs NULL: ELEMDP_EINVAL; a call
 * before elemdp_load_batch: ELEMDP_ESTATE; a list before any loop call on the resident batch: ELEMDP_ESTATE, with cap below the
 * length of the list: ELEMDP_EINVAL (its arrays may be NULL); no device: ELEMDP_ENODEV.  elemdp_last_timing afterwards: [whole
 * call, sum passes + loop kernels, sequences handed to the log-space form].  The other calls of the handle are unaffected; the lists
 * of the last pair, conditional, stem and helix call stay valid, and those calls leave the loop lists alone. */
#define ELEMDP_LOOP_H 1
#define ELEMDP_LOOP_S 2
#define ELEMDP_LOOP_B 3
#define ELEMDP_LOOP_I 4
#define ELEMDP_LOOP_M 5
int elemdp_loop_posteriors(elemdp_handle* h, const double* x, int32_t n_param, double min_prob, double* counts, int64_t* n_closing,
                           int64_t* n_two, const char* structure, int32_t* loop_type, double* loop_prob);
int elemdp_loop_closing_list(elemdp_handle* h, int32_t* seq, int32_t* i, int32_t* j, double* p, double* cols, int64_t cap);
int elemdp_loop_two_list(elemdp_handle* h, int32_t* seq, int32_t* i, int32_t* j, int32_t* k, int32_t* l, double* p, int64_t cap);
/* Accessibility under the motif model x: with U = max_width, access[U * (seq_off[n] + p) + (w - 1)], p 0-based,
 * w = 1 .. U, is the probability that the bases p .. p+w-1 of sequence n are all unpaired, over the ensemble of the scan's first sum
 * pass (terminals ari and nasi, Z(ari, nasi): the ensemble of elemdp_pair_posteriors and elemdp_context_profile), from its inside /
 * outside tables.  A window of unpaired bases lies in one maximal unpaired stretch, which the grammar makes by one of four chains of
 * single emissions -- a loop run (L <- L), the exterior (rule 8), the tail behind a multi-loop branch (rule 3a), the leading bases
 * of a multi-loop (rule 5a) -- and the value is the sum of the four w-step path sums between the tables, clamped to [0, 1]
 * (access_rules.h).  Width 1 is the unpaired vector of elemdp_pair_posteriors wherever the tables' inside and outside agree (1e-12
 * with energies at max_iloop 30); where the outside pass enumerates interior loops the inside pass does not -- max_iloop < 30, or a
 * model without energies on sequences longer than max_iloop -- the two cut the derivations at different items and differ by the
 * weight of those loops (2.5e-7 seen without energies at L = 40).  A window that runs off the end (p + w > L) is NaN.
 * A sequence without any parse (Z = 0) has 1 in every valid window, exactly, and so has every sequence under ELEMDP_NO_RSS.
 * Sequences that leave the double range of the scaled-linear tables, and every sequence under option pipeline 3, go through the
 * same rule on the log-space tables of the fused scan kernel.  max_width outside 1 .. 64, x NULL or access NULL is ELEMDP_EINVAL,
 * a call before elemdp_load_batch ELEMDP_ESTATE, a call without a device ELEMDP_ENODEV.  elemdp_last_timing afterwards: [whole call
 * including the copy to the host, sum passes + accessibility kernels, sequences handed to the log-space form].  Every buffer is
 * the call's own: elemdp_scan, the pair calls (the list of the last one stays valid), the other scan-family calls and the train
 * calls are unaffected. */
int elemdp_accessibility(elemdp_handle* h, const double* x, int32_t n_param, int32_t max_width, double* access);
/* Maximum expected accuracy motif alignments and site lists under the motif model x, decoded on the device from
 * the profile N of elemdp_node_profile.  A node row (0 = 'z' .. M-1 = 'o') is valid if it is the row of some alignment: all 'z', or
 * z^a n1^r1 .. nk^rk o^c over the pattern's nodes in order, r >= 1 (r >= 0 for a '*' node), the body not empty.  With g = gamma on
 * the pattern's nodes and 1 on 'z' and 'o', score(row) = sum_p g(row[p]) N(p, row[p]).  Slot 0 of a sequence is the valid row of
 * greatest score; the positions that carry its pattern nodes are one region [start, end), site 0.  Slot k is the best valid row that
 * puts no pattern node on a position of the sites 0 .. k-1; the list ends at the first slot whose best row is all 'z', or at
 * max_sites.  Sites of a sequence never overlap.  Ties go to the lower predecessor at every step and the lower final node: the
 * result is a function of the profile's bits.  The row maximises a sum of marginals and need not be a derivation of positive
 * probability (with self-loops in the model it may repeat nodes); site_conf shows it.
 *   profile: NULL, or as for elemdp_node_profile (then the profile is copied to the host, else it stays on the device);
 *   node: the row of slot k of sequence n (seq_off[n] = b, length L) at node + max_sites * b + k * L, the layout of elemdp_sample;
 *   n_sites[n]: the sites found; site_start, site_end, site_score (of the whole row) and site_conf (the mean of N(p, row[p])
 *   over the site) at [n * max_sites + k].  Unused slots hold start = end = -1, score = conf = NaN and a row of 'z'.
 * Any output may be NULL.  A sequence without any parse has n_sites 0, exactly.  gamma not finite or <= 0, max_sites outside
 * 1 .. 64, more than 255 pattern nodes or x NULL is ELEMDP_EINVAL, a call before elemdp_load_batch ELEMDP_ESTATE.
 * elemdp_last_timing afterwards: [whole call including the copies to the host, sum passes + node kernels + decode, sequences
 * handed to the log-space form].  elemdp_scan, the pair calls (the list of the last one stays valid), elemdp_sample,
 * elemdp_context_profile, elemdp_node_profile and the train calls are unaffected. */
int elemdp_node_mea(elemdp_handle* h, const double* x, int32_t n_param, double gamma, int32_t max_sites,
                    double* profile, uint8_t* node, int32_t* n_sites, int32_t* site_start, int32_t* site_end,
                    double* site_score, double* site_conf);

/* timing of the last train evaluation, measured with HIP events on the engine's stream:
 * ms[0] = whole evaluation, ms[1] = the DP pipeline only (all kernels of the inside/outside sweeps),
 * ms[2] = number of sequences the scaled-linear pipeline handed to the log-space pipeline (range check);
 * with n > 3 also ms[3] = 1 when the last train evaluation of the scaled-linear pipeline found the zeros of the dead entries kept
 * in its slots and stored none (option "own_slots"), else 0, and ms[4] = the table slots the handle holds; with n > 5 also ms[5] =
 * the number of entries in the record of options that the inner engines of a streamed batch replay (a state of the handle like
 * entries 3 and 4, no timing; for the tests: setting "world" again replaces its entry) */
int elemdp_last_timing(elemdp_handle* h, double* ms, int32_t n);
/* debug: summed shader-clock cycles per phase of the last train evaluation when option "profile" = 1:
 * pipeline 2: [stage, inside band, inside exterior, outside exterior, outside band, queue/other];
 * pipeline 4 (16 values): k4_in [setup, stage split operands, split products, item sums, unary phase],
 * k4_out [setup, stage, products, items inner, items left, items right, unary phase, statistics flush] */
int elemdp_debug_profile(elemdp_handle* h, double* cycles, int32_t n);
/* Host only: the shuffled negative of one sequence as `elem train` (without --no-shuffle) generates it per iteration:
 * k-let preserving Euler-tour shuffle (uShuffle, Jiang et al. 2007; RNAelem/ushuffle/ushuffle.c:139-290) driven by the C
 * library's srand(seed) / rand() exactly as RNAelem/motif_trainer.hpp:145-152 does (seed = occurrences of the first base
 * + iteration count).  codes / out: L base codes.  Not thread safe (rand() is process global). */
int elemdp_kmer_shuffle(const uint8_t* codes, int32_t L, int32_t k, int32_t iter_cnt, uint8_t* out);
/* Host only: the order in which `elem train --batch-size N` reads the records in epoch `seed`+1: the permutation that
 * std::shuffle(first, last, std::mt19937(seed)) applies to an array of n elements (FastqReader::shuffle,
 * RNAelem/fastq_io.hpp:115-124).  perm[i] = index (before the shuffle) of the element that ends at position i.  The
 * permutation is whatever the C++ standard library this library is built with produces -- the same one a reference
 * binary built with the same toolchain uses. */
int elemdp_epoch_permutation(int32_t n, int32_t seed, int32_t* perm);
/* name of the dominant kernel (for matching rocprofv3 rows) */
const char* elemdp_kernel_name(void);

#ifdef __cplusplus
}
#endif
#endif /* ELEMDP_H */
