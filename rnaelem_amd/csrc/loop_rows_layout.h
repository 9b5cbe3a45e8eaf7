// loop_rows_layout.h -- the dynamic LDS of k4_out_lrows (lin_kernels.hip): one function gives the kernel its
// regions and the launcher its byte count, so that the two cannot disagree, and lin_loop_outside_ok / group_geometry ask it whether
// an automaton and a band width fit.  Plain C++: host code and tests/loop_rows_layout_check.cpp include it as it is.
#pragma once

#if defined(__HIPCC__)
#define ELEMDP_LRL __host__ __device__ inline
#else
#define ELEMDP_LRL inline
#endif

namespace elemdp {

constexpr int kLoopRowsThreads = 256;   // threads of the workgroup (the band kernels' kBT)
constexpr int kLoopColsMax = 16;   // most columns of an L row the row kernels take (lin_loop_prepass_ok)
constexpr int kLoopProgW = 8;      // program words staged per column: P[0 .. 4 + kFastR)
constexpr int kRowsT = 8, kRowsMax = 32, kSeedCap = 256, kSeedBatch = 2;   // (kSeedCap: records staged at a time)
constexpr int kLoopRowsLdsMax = 64 * 1024;   // a workgroup's most: beyond it the sweep computes L itself

// rows of a workgroup: every lane has a chain entry, at most kRowsMax (which bounds the run tables)
ELEMDP_LRL int loop_rows_r(int rs) { const int r = kLoopRowsThreads / (rs > 0 ? rs : 1); return r < kRowsMax ? r : kRowsMax; }

struct LdsRegion { int off, bytes, align; };
struct LoopRowsLds {
  int rows, tiles, npos, nokw;   // rows R, tiles of kRowsT diagonals of a band of W, staged positions, staged pair-mask words
  LdsRegion acc;    // double [row][diagonal of the tile, + the parent row][column]: the tile's entries
  LdsRegion xw;     // double [2][kSeedCap]: exp(lambda_k tsc) of the staged records
  LdsRegion ew;     // double [npos]: position weight of i0 + .   (per workgroup)
  LdsRegion wr;     // double [5 n_wr]
  LdsRegion en;     // double [2 n_theta + 4]: the statistics of the two worlds
  LdsRegion lo;     // int [tile][2 R]: first record of the run (role, row) in the tile   (per workgroup)
  LdsRegion pre;    // int [tile][2 R + 1]: records of the tile's runs before   (per workgroup)
  LdsRegion srow;   // int [4][kSeedCap]: rows of the staged records' three operands and their cell's entries
  LdsRegion tq;     // int [2 roles][2 n_quad]: the column records of the tuples
  LdsRegion lcol;   // int [n_lane]: lane of the unary phase -> L column
  LdsRegion prog;   // int [kLoopColsMax][kLoopProgW]: the outside program of the state that owns the column
  LdsRegion pst;    // int [kLoopColsMax]: ... and that state
  LdsRegion okw;    // uint32 [nokw]: the pair-mask words of the bits cell(i0 - 1, 0) .. cell(i0 + R - 2, W)   (per workgroup)
  LdsRegion pb;     // uint8 [npos]: base of i0 + .   (per workgroup)
  LdsRegion ub;     // uint8 [d = 0 .. W][R]: mask bytes of the workgroup's cells, 0 beyond the sequence   (per workgroup)
  int total;
};
constexpr int kLoopRowsRegions = 15;

// rs: columns of an L row; W: the widest band of the launch
ELEMDP_LRL LoopRowsLds loop_rows_layout(int rs, int W, int n_wr, int n_theta, int n_quad, int n_lane) {
  LoopRowsLds y;
  const int R = loop_rows_r(rs);
  y.rows = R;
  y.tiles = W / kRowsT + 1;
  y.npos = R + W;
  y.nokw = (R * (W + 1) + 31) / 32 + 1;
  int o = 0;
  auto take = [&o](LdsRegion& g, int bytes, int align) {
    o = (o + align - 1) / align * align;
    g.off = o; g.bytes = bytes; g.align = align;
    o += bytes;
  };
  take(y.acc, 8 * R * (kRowsT + 1) * rs, 8);
  take(y.xw, 8 * 2 * kSeedCap, 8);
  take(y.ew, 8 * y.npos, 8);
  take(y.wr, 8 * 5 * n_wr, 8);
  take(y.en, 8 * (2 * n_theta + 4), 8);
  take(y.lo, 4 * y.tiles * 2 * R, 4);
  take(y.pre, 4 * y.tiles * (2 * R + 1), 4);
  take(y.srow, 4 * 4 * kSeedCap, 4);
  take(y.tq, 4 * 4 * n_quad, 4);
  take(y.lcol, 4 * n_lane, 4);
  take(y.prog, 4 * kLoopColsMax * kLoopProgW, 4);
  take(y.pst, 4 * kLoopColsMax, 4);
  take(y.okw, 4 * y.nokw, 4);
  take(y.pb, y.npos, 1);
  take(y.ub, R * (W + 1), 1);
  y.total = (o + 7) / 8 * 8;
  return y;
}
// the regions in layout order (tests)
inline void loop_rows_regions(const LoopRowsLds& y, LdsRegion out[kLoopRowsRegions]) {
  const LdsRegion all[kLoopRowsRegions] = {y.acc, y.xw, y.ew, y.wr, y.en, y.lo, y.pre, y.srow, y.tq, y.lcol, y.prog, y.pst, y.okw, y.pb, y.ub};
  for (int k = 0; k < kLoopRowsRegions; ++k) out[k] = all[k];
}
// the bytes the launcher passes for an automaton of these sizes at band width W, and whether the kernel takes it at all
ELEMDP_LRL int loop_rows_lds_bytes(int rs, int W, int n_wr, int n_theta, int n_quad, int n_lane) { return loop_rows_layout(rs, W, n_wr, n_theta, n_quad, n_lane).total; }
ELEMDP_LRL bool loop_rows_fits(int rs, int W, int n_wr, int n_theta, int n_quad, int n_lane) {
  return rs >= 1 && rs <= kLoopColsMax && rs <= kLoopRowsThreads && W >= 0 && loop_rows_lds_bytes(rs, W, n_wr, n_theta, n_quad, n_lane) <= kLoopRowsLdsMax;
}

}  // namespace elemdp
