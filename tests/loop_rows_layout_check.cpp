// Test-only driver of the LDS layout of k4_out_lrows (rnaelem_amd/csrc/loop_rows_layout.h): a stand-alone program, built by
// tests/test_loop_rows_layout_cpu.py with the address and undefined-behaviour sanitizers.  It checks by itself, prints one line per
// failed check and "ok <checks>" at the end; the exit status is the number of failures (at most 100).
#include <algorithm>
#include <cstdio>
#include <set>
#include <vector>

#include "../rnaelem_amd/csrc/loop_rows_layout.h"

using namespace elemdp;

static int n_checks = 0, n_failed = 0;
#define CHECK(cond, ...) do { ++n_checks; if (!(cond)) { ++n_failed; printf("FAILED %s:%d %s: ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } } while (0)

int main() {
  // columns of an L row: 1 .. 16 (what the kernel takes), and 32 and 256 for blocks of 8 rows and of one row
  std::vector<int> widths;
  for (int rs = 1; rs <= 16; ++rs) widths.push_back(rs);
  widths.push_back(32);
  widths.push_back(256);
  const int autos[3][4] = {{1, 1, 0, 1}, {3, 27, 5, 13}, {8, 54, 12, 22}};   // n_wr, n_theta, n_quad, n_lane
  std::set<int> rows_seen;
  for (int rs : widths)
    for (int W : {3, 50, 64, 120})
      for (const int* A : autos) {
        const LoopRowsLds y = loop_rows_layout(rs, W, A[0], A[1], A[2], A[3]);
        const int R = loop_rows_r(rs);
        rows_seen.insert(R);
        CHECK(y.rows == R && R >= 1 && R <= kRowsMax && R * rs <= kLoopRowsThreads, "rs %d: %d rows", rs, y.rows);
        LdsRegion g[kLoopRowsRegions];
        loop_rows_regions(y, g);
        std::vector<LdsRegion> v(g, g + kLoopRowsRegions);
        std::sort(v.begin(), v.end(), [](const LdsRegion& a, const LdsRegion& b) { return a.off < b.off; });
        int end = 0;
        for (int k = 0; k < kLoopRowsRegions; ++k) {
          CHECK(v[k].off >= end, "rs %d W %d: region at %d overlaps the one before, which ends at %d", rs, W, v[k].off, end);
          CHECK(v[k].align >= 1 && v[k].off % v[k].align == 0, "rs %d W %d: region at %d, alignment %d", rs, W, v[k].off, v[k].align);
          CHECK(v[k].bytes >= 0, "rs %d W %d: region of %d bytes", rs, W, v[k].bytes);
          end = v[k].off + v[k].bytes;
        }
        CHECK(end <= y.total && y.total % 8 == 0 && y.total - end < 8, "rs %d W %d: total %d, last region ends at %d", rs, W, y.total, end);
        for (const LdsRegion* d : {&y.acc, &y.xw, &y.ew, &y.wr, &y.en}) CHECK(d->align == 8, "doubles at %d", d->off);
        for (const LdsRegion* d : {&y.lo, &y.pre, &y.srow, &y.tq, &y.lcol, &y.prog, &y.pst, &y.okw}) CHECK(d->align == 4, "ints at %d", d->off);
        CHECK(y.pst.off == y.prog.off + y.prog.bytes, "the programs and their states are cleared as one run");
        // the launcher's byte count and the fit are this layout's
        CHECK(loop_rows_lds_bytes(rs, W, A[0], A[1], A[2], A[3]) == y.total, "rs %d W %d: the launcher passes %d", rs, W, loop_rows_lds_bytes(rs, W, A[0], A[1], A[2], A[3]));
        CHECK(loop_rows_fits(rs, W, A[0], A[1], A[2], A[3]) == (rs <= kLoopColsMax && y.total <= kLoopRowsLdsMax), "rs %d W %d: fits", rs, W);
        // what the kernel stores per workgroup fits its region, whatever the first row of the workgroup and the sequence's length
        CHECK(y.acc.bytes == 8 * R * (kRowsT + 1) * rs, "entries");
        CHECK(y.ub.bytes >= R * (W + 1), "mask bytes");
        CHECK(y.pb.bytes >= R + W && y.ew.bytes >= 8 * (R + W) && y.npos == R + W, "positions i0 .. i0 + R - 1 + W");
        CHECK(y.tiles * kRowsT >= W + 1 && y.lo.bytes == 4 * y.tiles * 2 * R && y.pre.bytes == 4 * y.tiles * (2 * R + 1), "%d tiles of a band of %d", y.tiles, W);
        CHECK(y.okw.bytes == 4 * y.nokw, "pair-mask words");
        for (int i0 = 0; i0 <= 3 * R + 40; i0 += (i0 < 40 ? 1 : R)) {
          const int first = (i0 > 0 ? (i0 - 1) * (W + 1) : 0) >> 5, last = std::max((i0 + R - 2) * (W + 1) + W, 0) >> 5;
          CHECK(last - first + 1 <= y.nokw, "rs %d W %d first row %d: %d words of the pair mask, room for %d", rs, W, i0, last - first + 1, y.nokw);
        }
      }
  for (int R : {1, 8, 16, 32}) CHECK(rows_seen.count(R) == 1, "no layout with blocks of %d rows was looked at", R);
  // the bench's shape -- 16 rows of 16 columns, W = 50 -- with an automaton of 54 parameters, 8 weight records, 12 tuples and 22
  // lanes: five workgroups per CU need 32 768 bytes or less each
  {
    const LoopRowsLds y = loop_rows_layout(16, 50, 8, 54, 12, 22);
    CHECK(y.rows == 16 && y.tiles == 7 && y.ub.bytes == 816 && y.nokw == 27, "the bench's shape: %d rows, %d tiles, %d mask bytes, %d words", y.rows, y.tiles, y.ub.bytes, y.nokw);
    CHECK(y.total <= 32768, "the bench's shape takes %d bytes", y.total);
  }
  // the band width decides: the same automaton falls back to the sweep where the staged plan data outgrow the workgroup's LDS
  CHECK(loop_rows_fits(13, 120, 8, 54, 12, 22), "W = 120 fits");
  CHECK(!loop_rows_fits(13, 2000, 8, 54, 12, 22), "W = 2000 does not fit");
  CHECK(!loop_rows_fits(17, 50, 8, 54, 12, 22) && !loop_rows_fits(0, 50, 8, 54, 12, 22), "rows of 17 columns and of none are not taken");
  printf("ok %d\n", n_checks - n_failed);
  return n_failed > 100 ? 100 : n_failed;
}
