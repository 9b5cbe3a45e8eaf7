// Test-only driver of the slot sizing arithmetic (rnaelem_amd/csrc/slot_sizing.h): a stand-alone program, built by
// tests/test_slot_sizing_cpu.py with the address and undefined-behaviour sanitizers.  Reads one case per line from stdin and
// answers one line per case:
//   S  S row scan n_want group opt_slots n_cu pair_row Lmax Wmax S_dense budget free held  have_n have_S have_band have_trace
//        -> want band ext dense1 per_slot keep sized
//   G  per_slot_bytes n group_cap opt_group budget free held      -> group size
//   E  n n_slots                                                  -> group size
//   B  Lmax Wmax row Sa nap                                       -> bytes per sequence of a scaled-linear group
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../rnaelem_amd/csrc/slot_sizing.h"

using namespace elemdp;

int main() {
  char line[1024];
  long n_lines = 0;
  while (fgets(line, sizeof(line), stdin)) {
    ++n_lines;
    const char kind = line[0];
    unsigned long long v[18];
    int n = 0;
    for (char* p = line + 1; n < 18;) {
      char* end = nullptr;
      v[n] = strtoull(p, &end, 10);
      if (end == p) break;
      ++n;
      p = end;
    }
    if (kind == 'S' && n == 18) {
      SlotRequest r;
      r.S = (int)v[0]; r.row = (int)v[1]; r.scan = v[2] != 0; r.n_want = (int)v[3]; r.group = (int)v[4];
      r.opt_slots = (int)v[5]; r.n_cu = (int)v[6]; r.pair_row = (int)v[7]; r.Lmax = (int)v[8]; r.Wmax = (int)v[9];
      r.S_dense = (int)v[10]; r.budget = (size_t)v[11];
      SlotGeometry g;
      g.n = (int)v[14]; g.S = (int)v[15]; g.band_stride = (size_t)v[16]; g.trace = v[17] != 0;
      printf("%d %zu %zu %zu %zu %d %d\n", r.want(), r.band(), r.ext(), r.dense1(), r.per_slot(), slots_keep(g, r) ? 1 : 0,
             slots_sized(r, (size_t)v[12], (size_t)v[13]));
    } else if (kind == 'G' && n == 7) {
      printf("%d\n", balanced_group((size_t)v[0], (int)v[1], (int)v[2], (int)v[3], (size_t)v[4], (size_t)v[5], (size_t)v[6]));
    } else if (kind == 'E' && n == 2) {
      printf("%d\n", even_groups((int)v[0], (long)v[1]));
    } else if (kind == 'B' && n == 5) {
      printf("%zu\n", lin_group_bytes((int)v[0], (int)v[1], (int)v[2], (int)v[3], (int)v[4]));
    } else {
      fprintf(stderr, "slots_check: bad line %ld: %s", n_lines, line);
      return 2;
    }
  }
  return 0;
}
