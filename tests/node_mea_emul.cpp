// Test-only CPU driver of the maximum expected accuracy motif alignments: the chain recursion, the traceback and
// the site extraction of node_mea_rules.h, the nodes serial where k_node_mea spreads them over the lanes, over the lists the engine
// builds (node_mea_lists_build).  Not part of the product.  With -DNODE_MEA_MAIN a stand-alone program for a sanitizer build.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../rnaelem_amd/csrc/node_mea_rules.h"

using namespace elemdp;

namespace {

// the K decodes of one sequence; outputs as elemdp_node_mea for one sequence.  Returns n_sites.
int decode(const char* names, int M, int L, const double* prof, double gamma, int K, uint8_t* rows, int32_t* start, int32_t* end,
           double* score, double* conf) {
  std::vector<int32_t> blob;
  node_mea_lists_build(names, M, &blob);
  const NodeMeaLists nl{blob.data(), M};
  std::vector<double> V(2 * (size_t)M);
  std::vector<uint8_t> bp((size_t)M * (L > 0 ? L : 1));
  std::vector<int32_t> s0(K), s1(K);
  int found = 0;
  bool done = L <= 0;
  for (int k = 0; k < K; ++k) {
    if (!done) {
      double* v[2] = {V.data(), V.data() + M};
      const bool b0 = node_mea_barred(s0.data(), s1.data(), found, 0);
      for (int m = 0; m < M; ++m) v[0][m] = node_mea_first(nl, gamma, prof, m, b0);
      for (int p = 1; p < L; ++p) {
        const bool barred = node_mea_barred(s0.data(), s1.data(), found, p);
        for (int m = 0; m < M; ++m) {
          int from;
          v[p & 1][m] = node_mea_step(nl, gamma, prof + (size_t)M * p, v[(p & 1) ^ 1], m, barred, &from);
          bp[(size_t)M * p + m] = (uint8_t)from;
        }
      }
      double sc;
      const int fin = node_mea_final(nl, v[(L - 1) & 1], &sc);
      if (fin == 0) {
        done = true;
      } else {
        const NodeMeaSite s = node_mea_trace(nl, L, prof, bp.data(), fin, sc, rows + (size_t)k * L);
        start[k] = s.start; end[k] = s.end; score[k] = s.score; conf[k] = s.conf;
        s0[found] = s.start; s1[found] = s.end;
        ++found;
      }
    }
    if (done) {
      for (int p = 0; p < L; ++p) rows[(size_t)k * L + p] = 0;
      const NodeMeaSite s = node_mea_no_site();
      start[k] = s.start; end[k] = s.end; score[k] = s.score; conf[k] = s.conf;
    }
  }
  return found;
}

}  // namespace

extern "C" {

// lo, first, last: 3 M ints
void emu_node_mea_lists(const char* names, int M, int32_t* out) {
  std::vector<int32_t> blob;
  node_mea_lists_build(names, M, &blob);
  std::memcpy(out, blob.data(), sizeof(int32_t) * blob.size());
}

// prof: M * L doubles, prof[M * p + m]; rows: K * L bytes; the other outputs K entries.  Returns n_sites, -1 for arguments
// elemdp_node_mea refuses.
int emu_node_mea_seq(const char* names, int M, int L, const double* prof, double gamma, int K, uint8_t* rows, int32_t* start,
                     int32_t* end, double* score, double* conf) {
  if (!(gamma > 0.) || !std::isfinite(gamma) || K < 1 || K > kNodeMeaMaxSites || M < 3 || M > kNodeMeaMaxNodes) return -1;
  return decode(names, M, L, prof, gamma, K, rows, start, end, score, conf);
}

}  // extern "C"

#ifdef NODE_MEA_MAIN
// random profiles (rows on the simplex) at L = 47 .. 107, K = 4, three patterns; checks that the sites are ordered regions within
// the sequence that do not overlap and that every row entry is a node
int main() {
  const char* pats[3] = {"z((.*.))o", "z(.....)o", "z.*.o"};
  unsigned long long state = 88172645463325252ull;
  auto rnd = [&] { state ^= state << 13; state ^= state >> 7; state ^= state << 17; return (double)(state >> 11) / 9007199254740992.; };
  long total = 0;
  for (int t = 0; t < 3; ++t) {
    const int M = (int)std::strlen(pats[t]), K = 4;
    for (int L = 47; L <= 107; ++L) {
      std::vector<double> prof((size_t)M * L);
      for (int p = 0; p < L; ++p) {
        double sum = 0.;
        for (int m = 0; m < M; ++m) sum += prof[(size_t)M * p + m] = rnd() * rnd();
        for (int m = 0; m < M; ++m) prof[(size_t)M * p + m] /= sum;
      }
      std::vector<uint8_t> rows((size_t)K * L);
      int32_t s0[4], s1[4];
      double sc[4], cf[4];
      const int ns = emu_node_mea_seq(pats[t], M, L, prof.data(), 4.0, K, rows.data(), s0, s1, sc, cf);
      if (ns < 0 || ns > K) { std::printf("bad n_sites %d\n", ns); return 1; }
      for (int k = 0; k < ns; ++k) {
        if (!(0 <= s0[k] && s0[k] < s1[k] && s1[k] <= L)) { std::printf("bad site\n"); return 1; }
        for (int j = 0; j < k; ++j)
          if (s0[k] < s1[j] && s0[j] < s1[k]) { std::printf("sites overlap\n"); return 1; }
      }
      for (size_t i = 0; i < rows.size(); ++i)
        if (rows[i] >= M) { std::printf("bad node\n"); return 1; }
      total += ns;
    }
  }
  std::printf("node_mea stand-alone: 3 patterns, L = 47 .. 107, K = 4, %ld sites, ok\n", total);
  return 0;
}
#endif
