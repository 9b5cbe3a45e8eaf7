"""Host-side mirror of the reference's operator interface, over the C ABI of libelemdp.so.

    RNAelemTrainer::operator()(x, fn, gr)   RNAelem/motif_trainer.hpp:595   ->  Engine.train_eval(x)
    RNAelemScanner::scan(model)             RNAelem/motif_scanner.hpp:938   ->  Engine.scan(x)

Only ctypes and numpy are used here; torch enters in rnaelem_amd/distributed.py for the RCCL
all-reduce.  There is no CPU fallback: if the library cannot be loaded or no GPU is present the
calls raise.
"""
import ctypes as C
import functools
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libelemdp.so")

NO_RSS, NO_PROFILE, NO_ENERGY, THETA_SOFTMAX, LIK_RATIO = 1, 2, 4, 8, 16
DBG_FIX_RSS, DBG_NO_TURN = 1 << 9, 1 << 10

# every symbol include/elemdp.h declares
SYMBOLS = ["elemdp_last_error", "elemdp_abi_version", "elemdp_set_data_dir", "elemdp_create", "elemdp_destroy",
           "elemdp_n_param", "elemdp_n_state", "elemdp_n_node", "elemdp_initial_params", "elemdp_describe",
           "elemdp_set_option", "elemdp_load_batch", "elemdp_load_batch_constrained", "elemdp_constraint_mask_host", "elemdp_batch_bpp_eff", "elemdp_batch_pairs", "elemdp_useful_mask", "elemdp_useful_mask_host", "elemdp_live_blocks", "elemdp_live_blocks_host", "elemdp_live_blocks_inside", "elemdp_live_blocks_host_bits", "elemdp_pair_terms", "elemdp_pair_terms_host", "elemdp_train_eval",
           "elemdp_partial_len", "elemdp_train_partial", "elemdp_train_finish", "elemdp_set_finish_params", "elemdp_train_seq_stats", "elemdp_train_seq_counts",
           "elemdp_debug_tables", "elemdp_scan", "elemdp_pair_posteriors", "elemdp_pair_mea", "elemdp_sample", "elemdp_context_profile", "elemdp_node_profile", "elemdp_joint_profile", "elemdp_stem_slots", "elemdp_stem_profile", "elemdp_stem_list", "elemdp_helix_posteriors", "elemdp_helix_list", "elemdp_loop_posteriors", "elemdp_loop_closing_list", "elemdp_loop_two_list", "elemdp_accessibility", "elemdp_node_mea", "elemdp_pair_conditional", "elemdp_pair_conditional_list", "elemdp_pair_list", "elemdp_last_timing", "elemdp_debug_profile", "elemdp_kernel_name", "elemdp_kmer_shuffle", "elemdp_epoch_permutation",
           "elemdp_comm_unique_id", "elemdp_comm_init", "elemdp_comm_destroy"]


class ModelDesc(C.Structure):
    _fields_ = [("pattern", C.c_char_p), ("energy_param", C.c_char_p), ("max_span", C.c_int32), ("max_iloop", C.c_int32),
                ("min_bpp", C.c_double), ("tau", C.c_double), ("flags", C.c_int32), ("device", C.c_int32)]


class ScanOut(C.Structure):
    _fields_ = [("start", C.POINTER(C.c_double)), ("end", C.POINTER(C.c_double)), ("inner", C.POINTER(C.c_double)),
                ("psihat", C.POINTER(C.c_int32)), ("rss", C.c_char_p), ("ys", C.POINTER(C.c_int32)),
                ("ye", C.POINTER(C.c_int32)), ("exist_prob", C.POINTER(C.c_double)), ("en", C.POINTER(C.c_double))]


class ElemdpError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("libelemdp error %d: %s" % (code, msg))
        self.code = code


_lib = None


def load_library():
    """dlopen libelemdp.so (fails loudly if it has not been built: there is no fallback)."""
    global _lib
    if _lib is None:
        # (ELEMDP_LIBRARY: another build of the same sources -- a timing variant, or the host-sanitizer build of tools/sanitize_cpu.sh)
        path = os.environ.get("ELEMDP_LIBRARY") or LIB_PATH
        if not os.path.exists(path):
            raise ElemdpError(-100, "%s is not built (run `python -m rnaelem_amd.build`)" % path)
        L = C.CDLL(path)
        dp, u8, i32 = C.POINTER(C.c_double), C.POINTER(C.c_uint8), C.POINTER(C.c_int32)
        hp = C.c_void_p
        L.elemdp_last_error.restype = C.c_char_p
        L.elemdp_kernel_name.restype = C.c_char_p
        L.elemdp_set_data_dir.argtypes = [C.c_char_p]
        if path != LIB_PATH:      # (the library looks for its energy parameter files next to itself)
            L.elemdp_set_data_dir(os.path.join(os.path.dirname(LIB_PATH), "data").encode())
        L.elemdp_create.argtypes = [C.POINTER(ModelDesc), C.POINTER(hp)]
        L.elemdp_destroy.argtypes = [hp]
        for f in ("elemdp_n_param", "elemdp_n_state", "elemdp_n_node", "elemdp_partial_len"):
            getattr(L, f).argtypes = [hp]
        L.elemdp_initial_params.argtypes = [hp, C.c_double, dp, C.c_int32]
        L.elemdp_describe.argtypes = [hp, C.c_char_p, C.c_int32]
        L.elemdp_set_option.argtypes = [hp, C.c_char_p, C.c_double]
        L.elemdp_load_batch.argtypes = [hp, u8, i32, u8, i32, C.c_char_p, C.c_int32]
        L.elemdp_load_batch_constrained.argtypes = [hp, u8, i32, u8, i32, C.c_char_p, C.c_int32]
        L.elemdp_constraint_mask_host.argtypes = [u8, u8, C.c_char_p, C.c_int32, C.c_int32, C.c_int32, u8, u8]
        L.elemdp_batch_bpp_eff.argtypes = [hp, dp, C.c_int32]
        L.elemdp_batch_pairs.argtypes = [hp, C.c_int32, u8, dp, C.c_int32]
        L.elemdp_useful_mask.argtypes = [hp, C.c_int32, u8, C.c_int32]
        L.elemdp_useful_mask_host.argtypes = [u8, u8, C.c_int32, C.c_int32, C.c_int32, C.c_int32, u8]
        L.elemdp_live_blocks.argtypes = [hp, C.c_int32, C.POINTER(C.c_int32), C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        L.elemdp_live_blocks_host.argtypes = [u8, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.c_void_p, C.c_int32]
        L.elemdp_live_blocks_inside.argtypes = L.elemdp_live_blocks.argtypes
        L.elemdp_live_blocks_host_bits.argtypes = [u8, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.c_void_p, C.c_int32]
        u64 = C.POINTER(C.c_uint64)
        L.elemdp_pair_terms.argtypes = [hp, C.c_int32, u64, u64, C.c_int32]
        L.elemdp_pair_terms_host.argtypes = [u8, u8, C.c_int32, C.c_int32, u64, u64]
        L.elemdp_train_eval.argtypes = [hp, dp, C.c_int32, dp, dp, dp, i32]
        L.elemdp_train_partial.argtypes = [hp, dp, C.c_int32, C.c_void_p, C.c_int32]
        L.elemdp_train_finish.argtypes = [hp, dp, dp, dp, dp, i32]
        L.elemdp_set_finish_params.argtypes = [hp, dp, C.c_int32]
        L.elemdp_train_seq_stats.argtypes = [hp, dp, C.c_int32]
        L.elemdp_train_seq_counts.argtypes = [hp, dp, C.c_int32]
        L.elemdp_debug_tables.argtypes = [hp] + [dp] * 7
        L.elemdp_scan.argtypes = [hp, dp, C.c_int32, C.POINTER(ScanOut)]
        L.elemdp_pair_posteriors.argtypes = [hp, dp, C.c_int32, C.c_double, C.POINTER(C.c_int64), dp]
        L.elemdp_pair_mea.argtypes = [hp, dp, C.c_int32, C.c_double, C.c_double, C.POINTER(C.c_int64), dp, C.c_char_p, dp]
        L.elemdp_sample.argtypes = [hp, dp, C.c_int32, C.c_int32, C.c_uint64, C.c_int64, C.c_char_p, C.POINTER(C.c_uint8), dp, i32]
        L.elemdp_context_profile.argtypes = [hp, dp, C.c_int32, dp]
        L.elemdp_node_profile.argtypes = [hp, dp, C.c_int32, dp]
        L.elemdp_joint_profile.argtypes = [hp, dp, C.c_int32, dp, dp]
        L.elemdp_stem_slots.argtypes = [hp, i32, i32, C.c_int32]
        L.elemdp_stem_profile.argtypes = [hp, dp, C.c_int32, C.c_double, dp, C.POINTER(C.c_int64)]
        L.elemdp_stem_list.argtypes = [hp, i32, i32, i32, i32, dp, C.c_int64]
        L.elemdp_helix_posteriors.argtypes = [hp, dp, C.c_int32, C.c_int32, C.c_int32, C.c_double, C.POINTER(C.c_int64), C.c_char_p, i32, dp]
        L.elemdp_helix_list.argtypes = [hp, i32, i32, i32, i32, dp, C.c_int64]
        L.elemdp_loop_posteriors.argtypes = [hp, dp, C.c_int32, C.c_double, dp, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_char_p, i32, dp]
        L.elemdp_loop_closing_list.argtypes = [hp, i32, i32, i32, dp, dp, C.c_int64]
        L.elemdp_loop_two_list.argtypes = [hp, i32, i32, i32, i32, i32, dp, C.c_int64]
        L.elemdp_accessibility.argtypes = [hp, dp, C.c_int32, C.c_int32, dp]
        L.elemdp_node_mea.argtypes = [hp, dp, C.c_int32, C.c_double, C.c_int32, dp, u8, i32, i32, i32, dp, dp]
        L.elemdp_pair_list.argtypes = [hp, i32, i32, i32, dp, C.c_int64]
        L.elemdp_pair_conditional.argtypes = [hp, dp, C.c_int32, C.c_double, C.c_double, C.POINTER(C.c_int64), dp, dp, dp, C.c_char_p,
                                              C.c_char_p, dp]
        L.elemdp_pair_conditional_list.argtypes = [hp, i32, i32, i32, dp, dp, C.c_int64]
        L.elemdp_last_timing.argtypes = [hp, dp, C.c_int32]
        L.elemdp_epoch_permutation.argtypes = [C.c_int32, C.c_int32, C.POINTER(C.c_int32)]
        L.elemdp_kmer_shuffle.argtypes = [C.POINTER(C.c_uint8), C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_uint8)]
        L.elemdp_debug_profile.argtypes = [hp, dp, C.c_int32]
        L.elemdp_comm_unique_id.argtypes = [C.c_char_p]
        L.elemdp_comm_init.argtypes = [hp, C.c_int32, C.c_int32, C.c_char_p]
        L.elemdp_comm_destroy.argtypes = [hp]
        _lib = L
    return _lib


def _dp(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))


def _u8(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint8))


def _i32(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def epoch_permutation(n, seed):
    """perm of std::shuffle(.., std::mt19937(seed)) on n elements (host; elemdp_epoch_permutation)."""
    perm = np.zeros(n, dtype=np.int32)
    rc = load_library().elemdp_epoch_permutation(int(n), int(seed), _i32(perm))
    if rc:
        raise ElemdpError(rc, "epoch_permutation")
    return perm


def kmer_shuffle(codes, k, iter_cnt):
    """Shuffled negative of one sequence (host; elemdp_kmer_shuffle)."""
    codes = np.ascontiguousarray(codes, dtype=np.uint8)
    out = np.zeros_like(codes)
    rc = load_library().elemdp_kmer_shuffle(_u8(codes), len(codes), int(k), int(iter_cnt), _u8(out))
    if rc:
        raise ElemdpError(rc, "kmer_shuffle")
    return out


CONSTRAINT_ALPHABET = ".x|<>()"


def check_constraints(constraints, lengths):
    """The constraint strings of a batch as one list of str, None entries made free ('.' per base).  ValueError: another count of
    strings than sequences, or a string of another length than its sequence (the concatenated form the library takes cannot show
    either; the library checks the characters, the balance and the forced pairs)."""
    if len(constraints) != len(lengths):
        raise ValueError("%d constraint strings for %d sequences" % (len(constraints), len(lengths)))
    out = []
    for k, (c, n) in enumerate(zip(constraints, lengths)):
        if c is None:
            c = "." * n
        if len(c) != n:
            raise ValueError("constraint of sequence %d: %d characters for a sequence of %d" % (k, len(c), n))
        out.append(c)
    return out


def constraint_mask_host(kept, seq, constraint, flags=0):
    """The pair mask and the "may be unpaired" flags of one sequence under a constraint string, on the CPU: kept[(L+1), (W+1)]
    (the filter's pairs, as Engine.pairs gives them), seq (base codes) -> (kept_out, unp[L+1])  (host; elemdp_constraint_mask_host)."""
    kept = np.ascontiguousarray(kept, dtype=np.uint8)
    seq = np.ascontiguousarray(seq, dtype=np.uint8)
    L, W = kept.shape[0] - 1, kept.shape[1] - 1
    if len(seq) != L:
        raise ValueError("constraint_mask_host: %d bases for a mask of %d" % (len(seq), L))
    out = np.zeros_like(kept)
    unp = np.zeros(L + 1, dtype=np.uint8)
    lib = load_library()
    rc = lib.elemdp_constraint_mask_host(_u8(kept), _u8(seq), constraint.encode(), L, W, int(flags), _u8(out), _u8(unp))
    if rc:
        raise ElemdpError(rc, lib.elemdp_last_error().decode())
    return out, unp


# planes of the usefulness mask (elemdp_useful_mask): bit of each plane
USEFUL_BITS = dict(P=1, E=2, M=4, B=8, A=16, S1=32, S2=64, L=128)


def useful_mask_host(kept, max_iloop=30, flags=0, unp=None):
    """Usefulness mask of one sequence on the CPU from its kept pairs, kept[(L+1), (W+1)] -> uint8 [(W+1), (L+1)] of
    USEFUL_BITS (host; elemdp_useful_mask_host)."""
    kept = np.ascontiguousarray(kept, dtype=np.uint8)
    L, W = kept.shape[0] - 1, kept.shape[1] - 1
    out = np.zeros((W + 1, L + 1), dtype=np.uint8)
    u = None if unp is None else _u8(np.ascontiguousarray(unp, dtype=np.uint8))
    rc = load_library().elemdp_useful_mask_host(_u8(kept), u, L, W, int(max_iloop), int(flags), _u8(out))
    if rc:
        raise ElemdpError(rc, "useful_mask_host")
    return out


# a record of the live-block lists (elemdp_live_blocks): 16 bytes
LIVE_INSIDE_BITS = 0x7f   # every mask bit but L (128): the cells the inside sweep behind the loop pre-pass computes
LIVE_BLOCK = np.dtype([("live", "<u8"), ("first", "<i2"), ("own_lo", "<i2"), ("own_end", "<i2"), ("count", "<i2")])


def _live_block_lists(counts, recs):
    """[d] -> list of blocks (first cell, [live cells], (own_lo, own_end)) from the records of elemdp_live_blocks*."""
    out = []
    for d in range(len(counts)):
        row = []
        for r in recs[d, :counts[d]]:
            first, live = int(r["first"]), int(r["live"])
            cells = [first + k for k in range(64) if (live >> k) & 1]
            assert len(cells) == int(r["count"])
            row.append((first, cells, (int(r["own_lo"]), int(r["own_end"]))))
        out.append(row)
    return out


def live_blocks_host(mask, cpb, cap, bits=None):
    """Live-block lists of one sequence on the CPU from a mask [(W+1), (L+1)] (any non-zero byte is a live cell): per diagonal d
    the blocks (first cell, [live cells], (own_lo, own_end)) of at most `cpb` live cells that span at most `cap` cells (host;
    elemdp_live_blocks_host).  cap < cpb is refused.  bits: the mask bits that make a cell live (elemdp_live_blocks_host_bits;
    LIVE_INSIDE_BITS = the lists of the inside sweep behind the loop pre-pass)."""
    mask = np.ascontiguousarray(mask, dtype=np.uint8)
    W, L = mask.shape[0] - 1, mask.shape[1] - 1
    stride = (L + cpb) // max(int(cpb), 1) if cpb >= 1 else 1
    counts = np.zeros(W + 1, dtype=np.int32)
    recs = np.zeros((W + 1, max(stride, 1)), dtype=LIVE_BLOCK)
    if bits is None:
        rc = load_library().elemdp_live_blocks_host(_u8(mask), L, W, int(cpb), int(cap), counts.ctypes.data_as(C.POINTER(C.c_int32)),
                                                    recs.ctypes.data_as(C.c_void_p), recs.shape[1])
    else:
        rc = load_library().elemdp_live_blocks_host_bits(_u8(mask), L, W, int(cpb), int(cap), int(bits),
                                                         counts.ctypes.data_as(C.POINTER(C.c_int32)), recs.ctypes.data_as(C.c_void_p), recs.shape[1])
    if rc:
        raise ElemdpError(rc, "live_blocks_host")
    return _live_block_lists(counts, recs)


def _u64(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint64))


def pair_terms_host(mask, kept):
    """Pair-term words of one sequence on the CPU from its mask [(W+1), (L+1)] and kept pairs [(L+1), (W+1)]: (ha_rows,
    h1_stems), uint64 [(W+1), (L+1)] each (host; elemdp_pair_terms_host).  W > 64 is refused."""
    mask = np.ascontiguousarray(mask, dtype=np.uint8)
    kept = np.ascontiguousarray(kept, dtype=np.uint8)
    W, L = mask.shape[0] - 1, mask.shape[1] - 1
    if kept.shape != (L + 1, W + 1):
        raise ValueError("pair_terms_host: kept must be [(L+1), (W+1)]")
    ha = np.zeros((W + 1, L + 1), dtype=np.uint64)
    h1 = np.zeros((W + 1, L + 1), dtype=np.uint64)
    rc = load_library().elemdp_pair_terms_host(_u8(mask), _u8(kept), L, W, _u64(ha), _u64(h1))
    if rc:
        raise ElemdpError(rc, "pair_terms_host")
    return ha, h1


HELIX_MAX_LEN = 32   # ELEMDP_HELIX_MAX_LEN


def _structure_mates(db):
    """mate[p] of every position of a dot-bracket string, -1 where unpaired (structure_mates of csrc/structure_rules.h)."""
    mate, stack = [-1] * len(db), []
    for p, c in enumerate(db):
        if c == "(":
            stack.append(p)
        elif c == ")":
            if not stack:
                raise ValueError("unbalanced structure")
            mate[p] = stack.pop()
            mate[mate[p]] = p
        elif c != ".":
            raise ValueError("a structure holds ( ) . only")
    if stack:
        raise ValueError("unbalanced structure")
    return mate


def structure_helices(db):
    """The stems of a dot-bracket string, host only: (i, j, len) per maximal run of directly nested pairs (i, j-1), (i+1, j-2), ..,
    i 0-based and j exclusive as in pair_posteriors, by increasing i.  Raises ValueError for an unbalanced string or one with
    characters other than ( ) ."""
    mate = _structure_mates(db)
    out = []
    for p, r in enumerate(mate):
        if r < p or (p > 0 and r + 1 < len(db) and mate[p - 1] == r + 1):
            continue
        n = 1
        while p + n < r - n and mate[p + n] == r - n:
            n += 1
        out.append((p, r + 1, n))
    return out


def stem_min_posterior(pairs, i, j, n):
    """The smallest pair posterior of the stem (i, j, n) in a pair list (i, j, p, ..) of its sequence; 0 where a pair is not listed."""
    ii, jj, pp = pairs[0], pairs[1], pairs[2]
    have = {(int(a), int(b)): float(v) for a, b, v in zip(ii, jj, pp)}
    return min(have.get((i + t, j - t), 0.0) for t in range(n))


LOOP_TYPES = " HSBIM"   # ELEMDP_LOOP_H .. ELEMDP_LOOP_M: the letter of loop type t is LOOP_TYPES[t]


def structure_loops(db):
    """The loops of a dot-bracket string, host only: (type, i, j, k, l) per pair, by increasing i.  The pair of the bases i and j-1
    (i 0-based and j exclusive as in pair_posteriors) closes a loop of type 1 .. 5 for H S B I M (LOOP_TYPES): a hairpin without an
    inner pair, a stack on the pair (i+1, j-1), a bulge with one inner pair and one empty side, an interior loop with one inner pair
    and bases on both sides, a multi-branch loop with two or more inner pairs.  (k, l) is the cell of the inner pair of a bulge or an
    interior loop, (-1, -1) otherwise.  Raises ValueError for an unbalanced string or one with characters other than ( ) ."""
    mate = _structure_mates(db)
    out = []
    for p, r in enumerate(mate):
        if r < p:
            continue
        inner, u = [], p + 1
        while u < r:
            if mate[u] > u:
                inner.append((u, mate[u]))
                u = mate[u] + 1
            else:
                u += 1
        if not inner:
            out.append((1, p, r + 1, -1, -1))
        elif len(inner) > 1:
            out.append((5, p, r + 1, -1, -1))
        elif inner[0] == (p + 1, r - 1):
            out.append((2, p, r + 1, -1, -1))
        else:
            k, l = inner[0]
            out.append((3 if (k == p + 1) != (l == r - 1) else 4, p, r + 1, k, l + 1))
    return out


WORLDS = ("mixed", "motif", "none")     # option "world": 0, 1, 2


def world_index(world):
    """0, 1, 2 for "mixed", "motif", "none" (or for the number itself); ValueError for anything else."""
    if isinstance(world, str) and world in WORLDS:
        return WORLDS.index(world)
    if not isinstance(world, (str, bool)) and world in (0, 1, 2):
        return int(world)
    raise ValueError("world: one of %s" % ", ".join(repr(w) for w in WORLDS))


def _in_world(method):
    """A posterior call that takes world="mixed" | "motif" | "none": the ensemble it describes -- the mixture of the parses with
    the motif and those without it (every call's default), the parses with the motif alone, or those without it alone (option
    "world").  The option is set for the call and put back afterwards, also when the call raises.  Without
    world= the call is the mixture's, whatever set_option("world", ..) left on the handle."""
    @functools.wraps(method)
    def call(self, *args, world="mixed", **kw):
        w = world_index(world)
        before = self._world
        if w == before:
            return method(self, *args, **kw)
        self.set_option("world", w)
        try:
            return method(self, *args, **kw)
        finally:
            self.set_option("world", before)
    return call


class Engine:
    """One model on one GPU (== one `RNAelem` object plus the trainer / scanner workers around it)."""

    def __init__(self, pattern, energy_param=None, max_span=50, max_iloop=30, min_bpp=1e-4, tau=0.1, flags=0, device=-1):
        self._lib = load_library()
        self._h = C.c_void_p()
        self._keep = (pattern.encode(), None if energy_param is None else energy_param.encode())
        d = ModelDesc(self._keep[0], self._keep[1], max_span, max_iloop, min_bpp, tau, flags, device)
        self._check(self._lib.elemdp_create(C.byref(d), C.byref(self._h)))
        self.flags = flags
        self.max_span = max_span
        self.n_param = self._lib.elemdp_n_param(self._h)
        self.n_state = self._lib.elemdp_n_state(self._h)
        self.n_node = self._lib.elemdp_n_node(self._h)
        self.n_seq = 0
        self._off = self._qoff = None
        self._world = 0

    @property
    def world(self):
        """The handle's option "world" as last set: the world a raw library call runs in.  The posterior methods of this class do
        not follow it -- each runs in its own world= argument, "mixed" when none is given, and puts this value back afterwards."""
        return WORLDS[self._world]

    def _check(self, rc):
        if rc < 0:
            raise ElemdpError(rc, self._lib.elemdp_last_error().decode())
        return rc

    def close(self):
        if getattr(self, "_h", None):
            self._lib.elemdp_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- model
    def initial_params(self, lambda_init=0.0):
        x = np.zeros(self.n_param)
        self._check(self._lib.elemdp_initial_params(self._h, lambda_init, _dp(x), self.n_param))
        return x

    def describe(self):
        buf = C.create_string_buffer(1 << 20)
        self._check(self._lib.elemdp_describe(self._h, buf, len(buf)))
        return json.loads(buf.value.decode())

    def set_option(self, key, value):
        self._check(self._lib.elemdp_set_option(self._h, key.encode(), float(value)))
        if key == "world":
            self._world = int(value)

    # ---- batch
    def load_batch(self, seqs, quals, fix_rss=None, constraints=None):
        """seqs: list of uint8 code arrays; quals: list of uint8 arrays with len(seq)+1 entries.  constraints: a hard structure
        constraint per sequence (a str over CONSTRAINT_ALPHABET, one character per base; None: free), or None for a plain load."""
        n = len(seqs)
        off = np.zeros(n + 1, dtype=np.int32)
        qoff = np.zeros(n + 1, dtype=np.int32)
        if n:
            off[1:] = np.cumsum([len(s) for s in seqs])
            qoff[1:] = np.cumsum([len(q) for q in quals])
        sc = np.ascontiguousarray(np.concatenate(seqs) if n else np.zeros(1), dtype=np.uint8)
        qc = np.ascontiguousarray(np.concatenate(quals) if n else np.zeros(1), dtype=np.uint8)
        fx = None if fix_rss is None else "".join(fix_rss).encode()
        if constraints is not None:
            if fix_rss is not None:
                raise ValueError("load_batch: constraints or fix_rss, not both")
            cs = "".join(check_constraints(constraints, [len(s) for s in seqs])).encode()
            self._check(self._lib.elemdp_load_batch_constrained(self._h, _u8(sc), _i32(off), _u8(qc), _i32(qoff), cs, n))
        else:
            self._check(self._lib.elemdp_load_batch(self._h, _u8(sc), _i32(off), _u8(qc), _i32(qoff), fx, n))
        self.n_seq, self._off, self._qoff = n, off, qoff

    def bpp_eff(self):
        out = np.zeros(self.n_seq)
        self._check(self._lib.elemdp_batch_bpp_eff(self._h, _dp(out), self.n_seq))
        return out

    def pairs(self, index, with_lnbpp=False):
        L = int(self._off[index + 1] - self._off[index])
        W = min(L, self.max_span)
        kept = np.zeros((L + 1, W + 1), dtype=np.uint8)
        ln = np.full((L + 1, W + 1), -np.inf) if with_lnbpp else None
        self._check(self._lib.elemdp_batch_pairs(self._h, index, _u8(kept), _dp(ln), kept.size))
        return kept, ln

    def useful_mask(self, index):
        """uint8 [(W+1), (L+1)] of USEFUL_BITS: the entries of sequence `index` the train sweeps compute."""
        L = int(self._off[index + 1] - self._off[index])
        W = min(L, self.max_span)
        out = np.zeros((W + 1, L + 1), dtype=np.uint8)
        self._check(self._lib.elemdp_useful_mask(self._h, index, _u8(out), out.size))
        return out

    def pair_terms(self, index):
        """(ha_rows, h1_stems), uint64 [(W+1), (L+1)] each: the pair-term words of sequence `index` (elemdp_pair_terms)."""
        L = int(self._off[index + 1] - self._off[index])
        W = min(L, self.max_span)
        ha = np.zeros((W + 1, L + 1), dtype=np.uint64)
        h1 = np.zeros((W + 1, L + 1), dtype=np.uint64)
        self._check(self._lib.elemdp_pair_terms(self._h, index, _u64(ha), _u64(h1), ha.size))
        return ha, h1

    def live_blocks(self, index, with_taken=False, inside=False):
        """The live-block lists of sequence `index` for the model's cells per block and the span of the current options:
        (lists, cpb, cap), lists as live_blocks_host gives them; with_taken: also a bool array [W+1], True where a train
        evaluation of the current options sweeps that diagonal from its list (False: consecutive cells).  inside: the second
        set, the lists of the inside sweep behind the loop pre-pass (elemdp_live_blocks_inside)."""
        L = int(self._off[index + 1] - self._off[index])
        W = min(L, self.max_span)
        stride = (L + 8) // 8
        counts = np.zeros(W + 1, dtype=np.int32)
        recs = np.zeros((W + 1, stride), dtype=LIVE_BLOCK)
        cc = np.zeros(2, dtype=np.int32)
        taken = np.zeros(W + 1, dtype=np.int32)
        ip = C.POINTER(C.c_int32)
        entry = self._lib.elemdp_live_blocks_inside if inside else self._lib.elemdp_live_blocks
        self._check(entry(self._h, index, counts.ctypes.data_as(ip), recs.ctypes.data_as(C.c_void_p),
                          stride, cc.ctypes.data_as(ip), taken.ctypes.data_as(ip)))
        out = (_live_block_lists(counts, recs), int(cc[0]), int(cc[1]))
        return out + (taken != 0,) if with_taken else out

    # ---- training: == RNAelemTrainer::operator()
    def train_eval(self, x):
        x = np.ascontiguousarray(x, dtype=np.float64)
        gr = np.zeros(self.n_param)
        fn, eff, nsk = C.c_double(), C.c_double(), C.c_int32()
        self._check(self._lib.elemdp_train_eval(self._h, _dp(x), self.n_param, C.byref(fn), _dp(gr), C.byref(eff),
                                                C.byref(nsk)))
        return fn.value, gr, eff.value, nsk.value

    def partial_len(self):
        return self._lib.elemdp_partial_len(self._h)

    def train_partial(self, x, out=None, device_ptr=None):
        """Local sums before the cross-rank reduction.  `device_ptr`: raw device address to write to."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        if device_ptr is not None:
            self._check(self._lib.elemdp_train_partial(self._h, _dp(x), self.n_param, C.c_void_p(device_ptr), 1))
            return None
        if out is None:
            out = np.zeros(self.partial_len())
        self._check(self._lib.elemdp_train_partial(self._h, _dp(x), self.n_param, out.ctypes.data_as(C.c_void_p), 0))
        return out

    def train_finish(self, reduced, x=None):
        reduced = np.ascontiguousarray(reduced, dtype=np.float64)
        if x is not None:
            x = np.ascontiguousarray(x, dtype=np.float64)
            self._check(self._lib.elemdp_set_finish_params(self._h, _dp(x), self.n_param))
        gr = np.zeros(self.n_param)
        fn, eff, nsk = C.c_double(), C.c_double(), C.c_int32()
        self._check(self._lib.elemdp_train_finish(self._h, _dp(reduced), C.byref(fn), _dp(gr), C.byref(eff), C.byref(nsk)))
        return fn.value, gr, eff.value, nsk.value

    # ---- in-library collective (RCCL) for hosts without torch.distributed
    @staticmethod
    def comm_unique_id():
        """128-byte id (ncclUniqueId) that rank 0 creates and hands to the other ranks"""
        buf = C.create_string_buffer(128)
        rc = load_library().elemdp_comm_unique_id(buf)
        if rc < 0:
            raise ElemdpError(rc, load_library().elemdp_last_error().decode())
        return buf.raw

    def comm_init(self, rank, world, uid):
        self._check(self._lib.elemdp_comm_init(self._h, rank, world, C.c_char_p(uid)))

    def comm_destroy(self):
        self._check(self._lib.elemdp_comm_destroy(self._h))

    def seq_stats(self):
        out = np.zeros((self.n_seq, 5))
        self._check(self._lib.elemdp_train_seq_stats(self._h, _dp(out), self.n_seq))
        return out

    def seq_counts(self):
        """Per sequence the expected counts of the last train_eval / train_partial: dict of ENo, ENx (n_seq, n_theta) and
        EHo, EHx (n_seq, 2), the reference's (o, x) terms in every mode (schedule 0 / 1, LIK_RATIO, deterministic, log space).
        Resident batches only (ESTATE while streaming, before an evaluation and after a scan-family call)."""
        nt = self.n_param - 2
        out = np.zeros((self.n_seq, 2 * nt + 4))
        self._check(self._lib.elemdp_train_seq_counts(self._h, _dp(out), self.n_seq))
        return dict(ENo=out[:, :nt], ENx=out[:, nt:2 * nt], EHo=out[:, 2 * nt:2 * nt + 2], EHx=out[:, 2 * nt + 2:])

    def debug_tables(self):
        assert self.n_seq == 1
        L = int(self._off[1])
        W = min(L, self.max_span)
        S, nt = self.n_state, self.n_param - 2
        ins = np.zeros((L + 1, W + 1, 7, S))
        outs = np.zeros((L + 1, W + 1, 7, S))
        io, oo = np.zeros((L + 1, S)), np.zeros((L + 1, S))
        ENo, ENx, EH = np.zeros(nt), np.zeros(nt), np.zeros(4)
        self._check(self._lib.elemdp_debug_tables(self._h, _dp(ins), _dp(outs), _dp(io), _dp(oo), _dp(ENo), _dp(ENx), _dp(EH)))
        return dict(inside=ins, outside=outs, inside_o=io, outside_o=oo, ENo=ENo, ENx=ENx, EHo=EH[:2], EHx=EH[2:])

    # ---- scanning: == RNAelemScanner::scan
    def scan(self, x):
        x = np.ascontiguousarray(x, dtype=np.float64)
        n, off, qoff = self.n_seq, self._off, self._qoff
        tot = int(off[-1])
        start, inner, end = np.zeros(tot), np.zeros(tot), np.zeros(int(qoff[-1]))
        psi = np.zeros(tot, dtype=np.int32)
        rss = C.create_string_buffer(tot + 1)
        ys, ye = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
        ex, en = np.zeros(n), np.zeros(self.n_param - 2)
        so = ScanOut(_dp(start), _dp(end), _dp(inner), _i32(psi), C.cast(rss, C.c_char_p), _i32(ys), _i32(ye), _dp(ex), _dp(en))
        self._check(self._lib.elemdp_scan(self._h, _dp(x), self.n_param, C.byref(so)))
        raw = rss.raw[:tot].decode()
        recs = []
        for k in range(n):
            a, b = int(off[k]), int(off[k + 1])
            recs.append(dict(start=start[a:b], inner=inner[a:b], end=end[int(qoff[k]):int(qoff[k + 1])], psihat=psi[a:b],
                             rss=raw[a:b], Ys=int(ys[k]), Ye=int(ye[k]), exist_prob=float(ex[k])))
        return recs, en

    # ---- base-pair posteriors under the motif model
    @_in_world
    def pair_posteriors(self, x, min_prob=0.0):
        """One entry per sequence: (i, j, p, unpaired) -- the cells (i, j = i + d) whose bases i and j-1 (0-based) pair with
        probability p >= min_prob, in (i, j) order, and the probability that each base is unpaired."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        off = self._off
        unp = np.zeros(max(int(off[-1]), 1))
        m = C.c_int64()
        self._check(self._lib.elemdp_pair_posteriors(self._h, _dp(x), self.n_param, float(min_prob), C.byref(m), _dp(unp)))
        return self._pair_lists(m.value, unp)

    def _pair_lists(self, n, unp):
        off = self._off
        seq, ii, jj = (np.zeros(max(n, 1), dtype=np.int32) for _ in range(3))
        p = np.zeros(max(n, 1))
        self._check(self._lib.elemdp_pair_list(self._h, _i32(seq), _i32(ii), _i32(jj), _dp(p), max(n, 1)))
        bounds = np.searchsorted(seq[:n], np.arange(self.n_seq + 1))
        return [(ii[a:b].copy(), jj[a:b].copy(), p[a:b].copy(), unp[int(off[k]):int(off[k + 1])].copy())
                for k, (a, b) in enumerate(zip(bounds[:-1], bounds[1:]))]

    # ---- maximum expected accuracy structures under the motif model
    @_in_world
    def mea_structures(self, x, gamma=1.0, min_prob=None):
        """(structures, scores, pairs): per sequence the nested structure of kept pairs ('(', ')', '.') that maximises the sum of
        2 gamma P over its pairs plus the sum of the unpaired probabilities over its unpaired bases, and that sum.  pairs: what
        pair_posteriors(x, min_prob) gives, from the same call, or None when min_prob is None (then no list is built)."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        off = self._off
        unp = np.zeros(max(int(off[-1]), 1))
        s = C.create_string_buffer(max(int(off[-1]), 1))
        sc = np.zeros(max(self.n_seq, 1))
        m = C.c_int64()
        mp = float("inf") if min_prob is None else float(min_prob)
        self._check(self._lib.elemdp_pair_mea(self._h, _dp(x), self.n_param, mp, float(gamma), C.byref(m), _dp(unp), s, _dp(sc)))
        raw = s.raw.decode("ascii")
        structs = [raw[int(off[k]):int(off[k + 1])] for k in range(self.n_seq)]
        return structs, sc[:self.n_seq].copy(), None if min_prob is None else self._pair_lists(m.value, unp)

    # ---- motif-conditional pair posteriors
    def conditional_pairs(self, x, min_prob=0.0, gamma=None):
        """One record per sequence: the fold with the motif and the fold without it.  i, j: the cells (i, j = i + d) with
        max(p_motif, p_none) >= min_prob in (i, j) order; p_motif, p_none: the probability that bases i and j-1 (0-based) pair
        given a parse with the motif / without it; unpaired_motif, unpaired_none: per base; exist_prob = Z(ari) / Z(ari, nasi);
        shift: the sum of |p_motif - p_none| over the kept pairs.  With gamma also structure_motif and structure_none, the
        maximum expected accuracy structure of each world.  A world without any parse has p = 0, unpaired = 1, an open
        structure and shift NaN."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        off = self._off
        npos, ns = max(int(off[-1]), 1), max(self.n_seq, 1)
        um, un = np.zeros(npos), np.zeros(npos)
        ex, sh = np.zeros(ns), np.zeros(ns)
        sm = C.create_string_buffer(npos) if gamma is not None else None
        sn = C.create_string_buffer(npos) if gamma is not None else None
        m = C.c_int64()
        self._check(self._lib.elemdp_pair_conditional(self._h, _dp(x), self.n_param, float(min_prob), 0.0 if gamma is None else float(gamma),
                                                      C.byref(m), _dp(ex), _dp(um), _dp(un), sm, sn, _dp(sh)))
        n = m.value
        seq, ii, jj = (np.zeros(max(n, 1), dtype=np.int32) for _ in range(3))
        pm, pn = np.zeros(max(n, 1)), np.zeros(max(n, 1))
        self._check(self._lib.elemdp_pair_conditional_list(self._h, _i32(seq), _i32(ii), _i32(jj), _dp(pm), _dp(pn), max(n, 1)))
        bounds = np.searchsorted(seq[:n], np.arange(self.n_seq + 1))
        recs = []
        for k, (a, b) in enumerate(zip(bounds[:-1], bounds[1:])):
            lo, hi = int(off[k]), int(off[k + 1])
            r = dict(i=ii[a:b].copy(), j=jj[a:b].copy(), p_motif=pm[a:b].copy(), p_none=pn[a:b].copy(),
                     unpaired_motif=um[lo:hi].copy(), unpaired_none=un[lo:hi].copy(), exist_prob=float(ex[k]), shift=float(sh[k]))
            if gamma is not None:
                r["structure_motif"] = sm.raw[lo:hi].decode("ascii")
                r["structure_none"] = sn.raw[lo:hi].decode("ascii")
            recs.append(r)
        return recs

    # ---- stochastic samples of derivations
    SAMPLED, NO_PARSE, REFUSED = 0, 1, 2

    @_in_world
    def sample_structures(self, x, n_samples, seed=0, index_base=0):
        """One entry per sequence: (rss, nodes, logp, status) -- n_samples derivations drawn with their probabilities under the
        model: rss the structure letters (O L R H B I M) of each sample, nodes an (n_samples, L) uint8 array of motif nodes
        (psihat), logp the log-probability of each derivation, status SAMPLED, NO_PARSE or REFUSED (a failed walk: its sample has blank
        rss, nodes 0 and logp NaN).  The draws depend on (seed, index_base + batch index, sample index) only."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        off = self._off
        n_samples = int(n_samples)
        nb = max(int(off[-1]) * max(n_samples, 0), 1)
        rss = C.create_string_buffer(nb)
        node = np.zeros(nb, dtype=np.uint8)
        logp = np.zeros(max(self.n_seq * max(n_samples, 0), 1))
        status = np.zeros(max(self.n_seq, 1), dtype=np.int32)
        self._check(self._lib.elemdp_sample(self._h, _dp(x), self.n_param, n_samples, int(seed) & (2 ** 64 - 1), int(index_base),
                                            rss, node.ctypes.data_as(C.POINTER(C.c_uint8)), _dp(logp), _i32(status)))
        raw = rss.raw.decode("ascii")
        out = []
        for k in range(self.n_seq):
            L, b = int(off[k + 1] - off[k]), int(off[k]) * n_samples
            out.append(([raw[b + t * L:b + (t + 1) * L] for t in range(n_samples)], node[b:b + n_samples * L].reshape(n_samples, L).copy(),
                        logp[k * n_samples:(k + 1) * n_samples].copy(), int(status[k])))
        return out

    # ---- structural context profiles
    CONTEXT_LETTERS = "OLRHBIM"

    @_in_world
    def context_profiles(self, x):
        """One (L, 7) array per sequence: the probability that each base is exterior (O), the left (L) or right (R) base of a
        pair, or unpaired in a hairpin (H), bulge (B), interior (I) or multi-branch (M) loop -- the marginals of the rss letters,
        in the column order of CONTEXT_LETTERS, over the ensemble of pair_posteriors and sample_structures.  Rows sum to 1."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        off = self._off
        n_pos = int(off[-1]) if off is not None else 0
        prof = np.zeros(max(7 * n_pos, 1))
        self._check(self._lib.elemdp_context_profile(self._h, _dp(x), self.n_param, _dp(prof)))
        return [prof[7 * int(off[k]):7 * int(off[k + 1])].reshape(-1, 7).copy() for k in range(self.n_seq)]

    # ---- posterior motif-node profiles
    @_in_world
    def node_profiles(self, x):
        """One (L, M) array per sequence, M = n_node: the probability that each base is emitted by each pattern node, in the node
        order of describe()["node"] (0 = 'z', M-1 = 'o': the numbering of psihat and of the sampler's node rows), over the
        ensemble of pair_posteriors, context_profiles and sample_structures.  Rows sum to 1."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        off = self._off
        M = self.n_node
        n_pos = int(off[-1]) if off is not None else 0
        prof = np.zeros(max(M * n_pos, 1))
        self._check(self._lib.elemdp_node_profile(self._h, _dp(x), self.n_param, _dp(prof)))
        return [prof[M * int(off[k]):M * int(off[k + 1])].reshape(-1, M).copy() for k in range(self.n_seq)]

    # ---- joint node-by-context posteriors and emission counts
    @_in_world
    def joint_profiles(self, x, profile=False):
        """counts, an (n, M, 7, 5) array: the expected number of emissions of each base (N A C G U) by each pattern node (the
        node order of node_profiles) under each structure letter (the column order of CONTEXT_LETTERS), per sequence, reduced on
        the device -- the table behind a motif logo (motif_logo).  With profile=True returns (counts, profiles): one (L, M, 7)
        array per sequence, the probability that a base is emitted by the node and carries the letter; its sum over the letters
        is node_profiles, its sum over the nodes context_profiles.  Else the profile stays on the device."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        off = self._off
        M, n = self.n_node, max(self.n_seq, 0)
        n_pos = int(off[-1]) if off is not None else 0
        counts = np.zeros(max(n * M * 35, 1))
        prof = np.zeros(max(7 * M * n_pos, 1)) if profile else None
        self._check(self._lib.elemdp_joint_profile(self._h, _dp(x), self.n_param, _dp(counts), _dp(prof)))
        counts = counts[:n * M * 35].reshape(n, M, 7, 5)
        if not profile:
            return counts
        return counts, [prof[7 * M * int(off[k]):7 * M * int(off[k + 1])].reshape(-1, M, 7).copy() for k in range(self.n_seq)]

    # ---- pair posteriors by motif node pair and the stem logo table
    def stem_slots(self):
        """A (K, 2) int array: the node pair (left, right) of every stem slot -- the distinct pairs of pattern nodes that a pair
        transition of the model emits jointly, in increasing (left, right) order (node indices as in node_profiles)."""
        if getattr(self, "_stem_slots", None) is None:      # (the pattern's: built once per engine)
            K = self._check(self._lib.elemdp_stem_slots(self._h, None, None, 0))
            left, right = (np.zeros(max(K, 1), dtype=np.int32) for _ in range(2))
            self._check(self._lib.elemdp_stem_slots(self._h, _i32(left), _i32(right), K))
            self._stem_slots = np.stack([left[:K], right[:K]], axis=1)
        return self._stem_slots.copy()

    @_in_world
    def stem_profiles(self, x, min_prob=np.inf):
        """counts, an (n, K, 5, 5) array: per sequence and stem slot (stem_slots) the expected number of pairs the slot emits with
        each left base and each right base (N A C G U), reduced on the device -- the table behind a stem logo (stem_logo).  With
        a finite min_prob returns (counts, lists): per sequence (i, j, slot, q), the entries with q >= min_prob in (i, j, slot)
        order, q the probability that bases i and j-1 (0-based) pair and the pair is emitted by that slot; the sum of q over the
        slots of a cell is the p of pair_posteriors.  At min_prob 0 the list holds every slot of every kept cell."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        K, n = len(self.stem_slots()), max(self.n_seq, 0)
        counts = np.zeros(max(n * K * 25, 1))
        m = C.c_int64()
        self._check(self._lib.elemdp_stem_profile(self._h, _dp(x), self.n_param, float(min_prob), _dp(counts), C.byref(m)))
        counts = counts[:n * K * 25].reshape(n, K, 5, 5)
        if not np.isfinite(min_prob):
            return counts
        m = m.value
        seq, ii, jj, kk = (np.zeros(max(m, 1), dtype=np.int32) for _ in range(4))
        q = np.zeros(max(m, 1))
        self._check(self._lib.elemdp_stem_list(self._h, _i32(seq), _i32(ii), _i32(jj), _i32(kk), _dp(q), max(m, 1)))
        bounds = np.searchsorted(seq[:m], np.arange(self.n_seq + 1))
        return counts, [(ii[a:b].copy(), jj[a:b].copy(), kk[a:b].copy(), q[a:b].copy()) for a, b in zip(bounds[:-1], bounds[1:])]

    # ---- helix posteriors
    @_in_world
    def helix_posteriors(self, x, min_prob=0.01, min_len=2, max_len=16, structures=None):
        """Per sequence (i, j, len, p): the helices -- runs of len directly stacked pairs (i, j), (i+1, j-1), .., cells as in
        pair_posteriors -- with min_len <= len <= max_len (at most HELIX_MAX_LEN) whose joint probability p reaches min_prob, in
        (i, j, len) order, over the ensemble of pair_posteriors; len 1 is its p.  At min_prob 0 every (kept cell, len) whose cells
        are all kept; at +inf no list (empty arrays).  With structures (one dot-bracket string per sequence) returns
        (lists, stems): per sequence (i, j, len, p) of every stem of its structure (structure_helices), p the joint probability of
        the whole stem, whatever its length; 0 where a pair of the stem is not a kept cell."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        off = self._off
        n_pos = int(off[-1]) if off is not None else 0
        db = slen = sprob = None
        if structures is not None:
            structures = [s if isinstance(s, str) else bytes(s).decode() for s in structures]
            if off is None or len(structures) != self.n_seq or any(len(s) != int(off[k + 1] - off[k]) for k, s in enumerate(structures)):
                raise ValueError("helix_posteriors: one structure per sequence, of its length")
            db = "".join(structures).encode()
            slen = np.zeros(max(n_pos, 1), dtype=np.int32)
            sprob = np.zeros(max(n_pos, 1))
        m = C.c_int64()
        self._check(self._lib.elemdp_helix_posteriors(self._h, _dp(x), self.n_param, int(max_len), int(min_len), float(min_prob), C.byref(m),
                                                      db, _i32(slen) if slen is not None else None, _dp(sprob)))
        m = m.value
        seq, ii, jj, kk = (np.zeros(max(m, 1), dtype=np.int32) for _ in range(4))
        p = np.zeros(max(m, 1))
        if np.isfinite(min_prob):
            self._check(self._lib.elemdp_helix_list(self._h, _i32(seq), _i32(ii), _i32(jj), _i32(kk), _dp(p), max(m, 1)))
        bounds = np.searchsorted(seq[:m], np.arange(self.n_seq + 1))
        lists = [(ii[a:b].copy(), jj[a:b].copy(), kk[a:b].copy(), p[a:b].copy()) for a, b in zip(bounds[:-1], bounds[1:])]
        if structures is None:
            return lists
        stems = []
        for k in range(self.n_seq):
            a, b = int(off[k]), int(off[k + 1])
            at = np.nonzero(slen[a:b])[0]
            ln = slen[a:b][at]
            # (the 3' end of the outermost pair, exclusive: the partner of base i in the caller's own string)
            jj_k = np.array([j for _, j, _ in structure_helices(structures[k])], dtype=np.int32).reshape(-1)
            stems.append((at.astype(np.int32), jj_k, ln.copy(), sprob[a:b][at].copy()))
        return lists, stems

    # ---- loop posteriors
    @_in_world
    def loop_posteriors(self, x, min_prob=0.01, structures=None, counts=True):
        """(closing, two, counts): what every pair closes and the two-loops, over the ensemble of pair_posteriors.  closing: per
        sequence (i, j, p, cols) -- the cells of the pair list of pair_posteriors(x, min_prob) with its p and an (n, 5) array of the
        probabilities that the pair closes a hairpin, stacks on (i+1, j-1), closes a bulge, an interior loop or a multi-branch loop
        (H S B I M), in (i, j) order.  two: per sequence (i, j, k, l, p) -- the pair (i, j) directly around the pair (k, l) with
        unpaired bases between them -- for every two-loop whose probability reaches min_prob, by outer cell in closing order.
        counts: (n_seq, 5) expected numbers of loops of each type over every kept cell.  At min_prob 0 every kept cell and every
        two-loop; at +inf no lists (empty arrays).  With structures (one dot-bracket string per sequence) returns
        (closing, two, counts, loops): per sequence (type, i, j, k, l, p) of every loop of its structure (structure_loops), p the
        probability of that loop with no threshold; 0 where its pair is not a kept cell.  counts False: no counts (None in
        their place), and only the outer cells whose pair posterior reaches min_prob are walked."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        off = self._off
        n_pos = int(off[-1]) if off is not None else 0
        db = ltype = lprob = None
        if structures is not None:
            structures = [s if isinstance(s, str) else bytes(s).decode() for s in structures]
            if off is None or len(structures) != self.n_seq or any(len(s) != int(off[k + 1] - off[k]) for k, s in enumerate(structures)):
                raise ValueError("loop_posteriors: one structure per sequence, of its length")
            db = "".join(structures).encode()
            ltype = np.zeros(max(n_pos, 1), dtype=np.int32)
            lprob = np.zeros(max(n_pos, 1))
        counts = np.zeros((max(self.n_seq, 1), 5)) if counts else None
        mc, mt = C.c_int64(), C.c_int64()
        self._check(self._lib.elemdp_loop_posteriors(self._h, _dp(x), self.n_param, float(min_prob),
                                                     _dp(counts) if counts is not None else None, C.byref(mc), C.byref(mt),
                                                     db, _i32(ltype) if ltype is not None else None, _dp(lprob)))
        mc, mt = mc.value, mt.value
        seq, ii, jj = (np.zeros(max(mc, 1), dtype=np.int32) for _ in range(3))
        p, cols = np.zeros(max(mc, 1)), np.zeros((max(mc, 1), 5))
        tseq, ti, tj, tk, tl = (np.zeros(max(mt, 1), dtype=np.int32) for _ in range(5))
        tp = np.zeros(max(mt, 1))
        if np.isfinite(min_prob):
            self._check(self._lib.elemdp_loop_closing_list(self._h, _i32(seq), _i32(ii), _i32(jj), _dp(p), _dp(cols), max(mc, 1)))
            self._check(self._lib.elemdp_loop_two_list(self._h, _i32(tseq), _i32(ti), _i32(tj), _i32(tk), _i32(tl), _dp(tp), max(mt, 1)))
        bounds = np.searchsorted(seq[:mc], np.arange(self.n_seq + 1))
        closing = [(ii[a:b].copy(), jj[a:b].copy(), p[a:b].copy(), cols[a:b].copy()) for a, b in zip(bounds[:-1], bounds[1:])]
        bounds = np.searchsorted(tseq[:mt], np.arange(self.n_seq + 1))
        two = [(ti[a:b].copy(), tj[a:b].copy(), tk[a:b].copy(), tl[a:b].copy(), tp[a:b].copy()) for a, b in zip(bounds[:-1], bounds[1:])]
        counts = counts[:self.n_seq] if counts is not None else None
        if structures is None:
            return closing, two, counts
        loops = []
        for k in range(self.n_seq):
            a = int(off[k])
            ls = structure_loops(structures[k])
            cols5 = [np.array([l[c] for l in ls], dtype=np.int32).reshape(-1) for c in range(5)]
            at = cols5[1]
            if not np.array_equal(ltype[a + at], cols5[0]):
                raise RuntimeError("loop_posteriors: the library and structure_loops parse sequence %d differently" % k)
            loops.append(tuple(cols5) + (lprob[a + at].copy(),))
        return closing, two, counts, loops

    # ---- accessibility
    @_in_world
    def accessibility(self, x, max_width=16):
        """One (L, U) array per sequence, U = max_width (1 .. 64): column w-1 of row p is the probability that the bases
        p .. p+w-1 are all unpaired, over the ensemble of pair_posteriors and context_profiles; NaN where the window runs off the
        end.  Column 0 is the unpaired vector of pair_posteriors (to 1e-12 with energies at max_iloop 30; where the outside pass
        enumerates interior loops the inside pass does not -- max_iloop < 30, no energies and L > max_iloop -- they differ by the
        weight of those loops, 2.5e-7 seen).  Engine option access_terms (bits 1 loop runs, 2 exterior, 4 tails behind a
        multi-loop branch, 8 leading bases of a multi-loop; default 15) leaves terms out of the sum."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        off = self._off
        U = int(max_width)
        n_pos = int(off[-1]) if off is not None else 0
        acc = np.zeros(max(max(U, 1) * n_pos, 1))
        self._check(self._lib.elemdp_accessibility(self._h, _dp(x), self.n_param, U, _dp(acc)))
        return [acc[U * int(off[k]):U * int(off[k + 1])].reshape(-1, U).copy() for k in range(self.n_seq)]

    # ---- maximum expected accuracy motif alignments and site lists
    @_in_world
    def mea_alignments(self, x, gamma=1.0, max_sites=1, profile=False):
        """One dict per sequence, decoded on the device from the node profile: rows (n_sites, L) uint8 -- row k is the valid node
        row of greatest score sum_p g N(p, row[p]), g = gamma on the pattern's nodes and 1 on 'z' and 'o', that puts no pattern
        node on a position of the sites before it --, start, end (the region that carries the pattern's nodes), score (of the
        whole row) and confidence (the mean of N(p, row[p]) over the site), n_sites entries each; with profile=True also
        profile, the (L, M) array of node_profiles from the same call (else the profile stays on the device)."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        off = self._off
        M, K, n = self.n_node, int(max_sites), max(self.n_seq, 0)
        n_pos = int(off[-1]) if off is not None else 0
        kk = min(max(K, 1), 64)
        prof = np.zeros(max(M * n_pos, 1)) if profile else None
        node = np.zeros(max(kk * n_pos, 1), dtype=np.uint8)
        ns = np.zeros(max(n, 1), dtype=np.int32)
        s0, s1 = np.zeros(max(n * kk, 1), dtype=np.int32), np.zeros(max(n * kk, 1), dtype=np.int32)
        sc, cf = np.zeros(max(n * kk, 1)), np.zeros(max(n * kk, 1))
        self._check(self._lib.elemdp_node_mea(self._h, _dp(x), self.n_param, float(gamma), K, _dp(prof), _u8(node), _i32(ns),
                                              _i32(s0), _i32(s1), _dp(sc), _dp(cf)))
        out = []
        for k in range(self.n_seq):
            a, b, m = int(off[k]), int(off[k + 1]), int(ns[k])
            L = b - a
            rec = dict(rows=node[K * a:K * a + m * L].reshape(m, L).copy(), start=s0[k * K:k * K + m].copy(),
                       end=s1[k * K:k * K + m].copy(), score=sc[k * K:k * K + m].copy(), confidence=cf[k * K:k * K + m].copy())
            if profile:
                rec["profile"] = prof[M * a:M * b].reshape(L, M).copy()
            out.append(rec)
        return out

    def last_timing(self):
        """[ms whole evaluation, ms DP pipeline, sequences re-evaluated in log space]"""
        ms = np.zeros(3)
        self._lib.elemdp_last_timing(self._h, _dp(ms), 3)
        return ms

    def slot_status(self):
        """{"zeros_kept": the last train evaluation found the zeros of the dead entries kept in its table slots and stored none
        (option own_slots), "slots": table slots the handle holds}"""
        ms = np.zeros(5)
        self._lib.elemdp_last_timing(self._h, _dp(ms), 5)
        return {"zeros_kept": bool(ms[3]), "slots": int(ms[4])}

    def options_logged(self):
        """entries in the record of options the inner engines of a streamed batch replay (elemdp_last_timing entry 5)"""
        ms = np.zeros(6)
        self._lib.elemdp_last_timing(self._h, _dp(ms), 6)
        return int(ms[5])

    def profile(self):
        c = np.zeros(16)
        self._lib.elemdp_debug_profile(self._h, _dp(c), 16)
        return c

    def kernel_name(self):
        return self._lib.elemdp_kernel_name().decode()


def alignment_confidence(profile, psihat):
    """Confidence of a CYK alignment: N(p, psihat[p]) for every position p, from the (L, M) node profile of the sequence
    (Engine.node_profiles) and the node row the scan prints for it."""
    profile = np.asarray(profile, dtype=np.float64)
    psihat = np.asarray(psihat, dtype=np.int64)
    if profile.ndim != 2 or psihat.shape != (profile.shape[0],):
        raise ValueError("alignment_confidence: an (L, M) profile and L node indices are expected")
    if psihat.size and (psihat.min() < 0 or psihat.max() >= profile.shape[1]):
        raise ValueError("alignment_confidence: node index out of range")
    return profile[np.arange(profile.shape[0]), psihat]


def motif_logo(counts, weights=None):
    """The table behind a motif logo from the (n, M, 7, 5) counts of Engine.joint_profiles: the counts are summed over the
    sequences in input order, each times its weight if weights are given.  Returns a dict of arrays over the M pattern nodes:
    counts (M, 7, 5), the weighted sum; occurrences (M,), the expected number of bases the node emits; base_freq (M, 4), the
    frequencies of A C G U among the emissions with a known base; letter_freq (M, 7), the frequencies of the structure letters
    O L R H B I M; information (M,), 2 - H2 of base_freq in bits.  A node that emits nothing has frequencies and information 0.
    There is no small-sample correction: the counts are expectations, not a sample."""
    counts = np.asarray(counts, dtype=np.float64)
    if counts.ndim != 4 or counts.shape[2:] != (7, 5):
        raise ValueError("motif_logo: (n, M, 7, 5) counts are expected")
    n, M = counts.shape[:2]
    if weights is None:
        w = np.ones(n)
    else:
        w = np.asarray(weights, dtype=np.float64)
        if w.shape != (n,):
            raise ValueError("motif_logo: one weight per sequence is expected")
    total = np.zeros((M, 7, 5))
    for k in range(n):
        total += w[k] * counts[k]
    occ = total.sum(axis=(1, 2))
    known = total[:, :, 1:].sum(axis=1)
    ksum = known.sum(axis=1)
    base = np.divide(known, ksum[:, None], out=np.zeros_like(known), where=ksum[:, None] > 0)
    letters = total.sum(axis=2)
    letter = np.divide(letters, occ[:, None], out=np.zeros_like(letters), where=occ[:, None] > 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        h2 = -np.where(base > 0, base * np.log2(np.where(base > 0, base, 1.0)), 0.0).sum(axis=1)
    info = np.where(ksum > 0, 2.0 - h2, 0.0)
    return dict(counts=total, occurrences=occ, base_freq=base, letter_freq=letter, information=info)


STEM_PAIR_TYPES = ("CG", "GC", "GU", "UG", "AU", "UA")     # the order of a ')' node's theta row


def stem_logo(counts, slots, names, weights=None):
    """The table behind a stem logo from the (n, K, 5, 5) counts of Engine.stem_profiles, the (K, 2) slots of Engine.stem_slots
    and the node names (Engine.describe()["node"]): the counts are summed over the sequences in input order, each times its
    weight if weights are given.  Returns a dict of arrays over the K slots: counts (K, 5, 5), the weighted sum; labels, the two
    node names of each slot as '<left index><name>-<right index><name>'; occurrences (K,), the expected number of pairs the slot
    emits; pair_freq (K, 7), the frequencies of the six canonical pair types in the order of STEM_PAIR_TYPES, then "other" (any
    other two bases, N included); information (K,), log2(6) - H2 of the six canonical frequencies renormalised, in bits;
    mutual_information (K,), that of the left and the right column in bits, from the 4 x 4 block over A C G U.  A slot that
    emits nothing has frequencies, information and mutual information 0.  There is no small-sample correction: the counts are
    expectations, not a sample."""
    counts = np.asarray(counts, dtype=np.float64)
    slots = np.asarray(slots, dtype=np.int64).reshape(-1, 2)
    if counts.ndim != 4 or counts.shape[2:] != (5, 5) or counts.shape[1] != len(slots):
        raise ValueError("stem_logo: (n, K, 5, 5) counts and (K, 2) slots are expected")
    n, K = counts.shape[:2]
    if weights is None:
        w = np.ones(n)
    else:
        w = np.asarray(weights, dtype=np.float64)
        if w.shape != (n,):
            raise ValueError("stem_logo: one weight per sequence is expected")
    if len(slots) and (slots.min() < 0 or slots.max() >= len(names)):
        raise ValueError("stem_logo: node index out of range")
    total = np.zeros((K, 5, 5))
    for k in range(n):
        total += w[k] * counts[k]
    occ = total.sum(axis=(1, 2))
    code = {c: b for b, c in enumerate("NACGU")}
    canon = np.stack([total[:, code[t[0]], code[t[1]]] for t in STEM_PAIR_TYPES], axis=1) if K else np.zeros((0, 6))
    types = np.concatenate([canon, (occ - canon.sum(axis=1))[:, None]], axis=1)
    freq = np.divide(types, occ[:, None], out=np.zeros_like(types), where=occ[:, None] > 0)
    freq = np.maximum(freq, 0.0)          # (the remainder may round below 0)
    csum = canon.sum(axis=1)
    f6 = np.divide(canon, csum[:, None], out=np.zeros_like(canon), where=csum[:, None] > 0)

    def entropy(f):
        return -np.where(f > 0, f * np.log2(np.where(f > 0, f, 1.0)), 0.0)

    info = np.where(csum > 0, np.log2(6.0) - entropy(f6).sum(axis=1), 0.0)
    known = total[:, 1:, 1:]
    ksum = known.sum(axis=(1, 2))
    joint = np.divide(known, ksum[:, None, None], out=np.zeros_like(known), where=ksum[:, None, None] > 0)
    mi = entropy(joint.sum(axis=2)).sum(axis=1) + entropy(joint.sum(axis=1)).sum(axis=1) - entropy(joint).sum(axis=(1, 2))
    mi = np.where(ksum > 0, np.maximum(mi, 0.0), 0.0)
    labels = ["%d%s-%d%s" % (l, names[l], r, names[r]) for l, r in slots]
    return dict(counts=total, labels=labels, occurrences=occ, pair_freq=freq, information=info, mutual_information=mi)
