// Test-only driver of the own-slot sizing, the slot mapping and the zero binding (rnaelem_amd/csrc/slot_sizing.h): a stand-alone
// program, built by tests/test_own_slots_cpu.py with the address and undefined-behaviour sanitizers.  It checks by itself, prints
// one line per failed check and "ok <checks>" at the end; the exit status is the number of failures (at most 100).
#include <cstdio>
#include <vector>

#include "../rnaelem_amd/csrc/slot_sizing.h"

using namespace elemdp;

static int n_checks = 0, n_failed = 0;
#define CHECK(cond, ...) do { ++n_checks; if (!(cond)) { ++n_failed; printf("FAILED %s:%d %s: ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } } while (0)

// the group size of a sweep as Engine::sweep_groups computed it before stream_group had a place of its own
static int old_sweep_gsz(int n, int gsz, int n_slots, int ns) {
  const int slots_each = n_slots / ns;
  if (ns > 1) {
    int n_groups = (n + slots_each - 1) / slots_each;
    n_groups = ((n_groups + ns - 1) / ns) * ns;
    gsz = (n + n_groups - 1) / n_groups;
  }
  return gsz;
}

static ZeroBinding some_binding() {
  ZeroBinding z;
  z.valid = true; z.plan = 7; z.slots_gen = 3; z.n_slots = 24; z.band_stride = 1000; z.own = 1; z.n_seq = 24;
  z.S = 23; z.tab_row = 64; z.ap_rs = 12; z.shadow = 22; z.schedule = 1;
  z.useful_mask = 1; z.loop_prepass = 1; z.loop_outside = 1; z.live_blocks = 1; z.live_span = 32; z.deterministic = 0; z.fast = 1;
  return z;
}

int main() {
  // ---- fits or does not fit, around the edge of every rule (reach 1000 bytes: 680 for the groups, 720 for the slots)
  CHECK(own_slots_fit(680, 1, 1, 0, 0, 0, 1000, 0, 0), "the 68 %% rule, at the edge");
  CHECK(!own_slots_fit(681, 1, 1, 0, 0, 0, 1000, 0, 0), "the 68 %% rule, one past");
  CHECK(own_slots_fit(360, 1, 2, 0, 0, 0, 1000, 0, 0), "the 72 %% rule, at the edge");
  CHECK(!own_slots_fit(361, 1, 2, 0, 0, 0, 1000, 0, 0), "the 72 %% rule, one past");
  CHECK(own_slots_fit(100, 1, 1, 0, 0, 100, 1000, 0, 0), "an inner handle's budget, at the edge");
  CHECK(!own_slots_fit(101, 1, 1, 0, 0, 100, 1000, 0, 0), "an inner handle's budget, one past");
  CHECK(own_slots_fit(680, 1, 1, 0, 0, 0, 0, 1000, 1000), "held memory counts as within reach");
  CHECK(!own_slots_fit(680, 1, 1, 0, 0, 0, 0, 999, 1000), "each rule its own held set (groups)");
  CHECK(!own_slots_fit(360, 1, 2, 0, 0, 0, 0, 1000, 998), "each rule its own held set (slots)");
  CHECK(!own_slots_fit(0, 1, 1, 0, 0, 0, 1000, 0, 0), "no sequence");
  CHECK(own_slots_fit(24, 1, 1, 24, 0, 0, 1000, 0, 0) && !own_slots_fit(24, 1, 1, 23, 0, 0, 1000, 0, 0), "option group below the batch");
  CHECK(own_slots_fit(24, 1, 1, 0, 24, 0, 1000, 0, 0) && !own_slots_fit(24, 1, 1, 0, 23, 0, 1000, 0, 0), "option slots below the batch");
  {   // the bench shape on 288 GB: 10 000 sequences fit, 60 000 do not
    SlotRequest r;
    r.S = 23; r.row = 64; r.Lmax = 200; r.Wmax = 50; r.S_dense = 22; r.n_cu = 256; r.pair_row = 12;
    const size_t per = lin_group_bytes(200, 50, 64, 23, 12), GB = (size_t)1 << 30;
    CHECK(own_slots_fit(10000, per, r.per_slot(), 0, 0, 0, 288 * GB, 0, 0), "10 000 x L = 200 on 288 GB");
    CHECK(!own_slots_fit(60000, per, r.per_slot(), 0, 0, 0, 288 * GB, 0, 0), "60 000 x L = 200 on 288 GB");
  }

  // ---- the binding: it matches itself; not valid on either side, or any one field changed, breaks the match
  {
    const ZeroBinding z = some_binding();
    CHECK(zeros_match(z, z), "a binding matches itself");
    CHECK(!zeros_match(ZeroBinding(), ZeroBinding()), "two empty records do not match");
    std::vector<ZeroBinding> v(19, z);
    int k = 0;
    v[k++].valid = false; v[k++].plan += 1; v[k++].slots_gen += 1; v[k++].n_slots += 1; v[k++].band_stride += 1; v[k++].own = 0;
    v[k++].n_seq += 1; v[k++].S += 1; v[k++].tab_row += 1; v[k++].ap_rs += 1; v[k++].shadow = -1; v[k++].schedule = 0;
    v[k++].useful_mask = 0; v[k++].loop_prepass = 0; v[k++].loop_outside = 0; v[k++].live_blocks = 2; v[k++].live_span = 16;
    v[k++].deterministic = 1; v[k++].fast = 0;
    CHECK(k == (int)v.size(), "%d fields changed", k);
    for (int f = 0; f < k; ++f) {
      CHECK(!zeros_match(z, v[f]), "field %d of the wanted binding", f);
      CHECK(!zeros_match(v[f], z), "field %d of the held binding", f);
    }
  }

  // ---- the groups of a sweep are what they were, with or without a slot per sequence; the slots of the groups
  {
    const size_t per = lin_group_bytes(200, 50, 64, 23, 12), GB = (size_t)1 << 30;
    for (int n : {64, 5000, 10000, 60000})
      for (int ns : {1, 2, 4}) {
        const int group = balanced_group(per, n, 8192, 0, 0, 288 * GB, 0);
        SlotRequest r;
        r.S = 23; r.row = 64; r.Lmax = 200; r.Wmax = 50; r.S_dense = 22; r.n_cu = 256; r.pair_row = 12; r.n_want = n; r.group = group;
        const int n_shared = slots_sized(r, 288 * GB, 0);   // the slots of the shared mapping
        const int old = old_sweep_gsz(n, even_groups(n, n_shared), n_shared, ns);
        // the shared mapping through the new functions
        const int lock0 = lockstep_slots(false, group, n, n_shared);
        CHECK(stream_group(n, even_groups(n, lock0), lock0, ns) == old, "shared mapping: n %d ns %d", n, ns);
        // a slot per sequence: n slots
        const int lock1 = lockstep_slots(true, group, n, n);
        const int gsz = stream_group(n, even_groups(n, lock1), lock1, ns);
        CHECK(gsz == old, "a slot per sequence: n %d ns %d: groups of %d, were %d", n, ns, gsz, old);
        std::vector<char> used((size_t)n, 0);
        bool inside = true, once = true, shared_inside = true;
        int gi = 0;
        for (int g0 = 0; g0 < n; g0 += gsz, ++gi) {
          const int G = std::min(gsz, n - g0), k = gi % ns;
          const size_t b1 = group_slot_base(true, g0, k, lock1 / ns), b0 = group_slot_base(false, g0, k, lock0 / ns);
          for (int s = 0; s < G; ++s) {
            if (b1 + s >= (size_t)n) { inside = false; continue; }
            if (used[b1 + s]) once = false;
            used[b1 + s] = 1;
          }
          if (b0 != (size_t)k * (lock0 / ns) || b0 + G > (size_t)n_shared) shared_inside = false;
        }
        bool all = true;
        for (char u : used) all = all && u;
        CHECK(inside && once && all, "a slot per sequence: n %d ns %d: every slot 0 .. n - 1 taken by exactly one group (%d %d %d)", n, ns, inside, once, all);
        CHECK(shared_inside, "shared mapping: n %d ns %d: the groups of stream k stay inside its share of the slots", n, ns);
      }
  }
  printf("ok %d\n", n_checks - n_failed);
  return n_failed > 100 ? 100 : n_failed;
}
