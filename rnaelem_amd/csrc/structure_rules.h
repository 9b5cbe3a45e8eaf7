// structure_rules.h -- the dot-bracket structures a caller hands to helix_posteriors and loop_posteriors: the one parser and what
// it is read for, the stems and the loops (pure host functions, no device code; api.structure_helices and api.structure_loops
// state the same rules in Python, tests/structure_check.cpp runs these against them).
// (The FIX_RSS parser of stage_batch and constraint_derive stay on their own: other alphabets, messages and by-products.)
#pragma once
#include <cstdint>
#include <vector>

namespace elemdp {

// mate[p] of every position of db[0 .. L): the partner of a paired base, -1 of an unpaired one.  Returns "" or what is wrong.
inline const char* structure_mates(const char* db, int L, int32_t* mate) {
  std::vector<int32_t> open;
  for (int p = 0; p < L; ++p) {
    mate[p] = -1;
    if (db[p] == '(') open.push_back(p);
    else if (db[p] == ')') {
      if (open.empty()) return "unbalanced structure";
      mate[p] = open.back(); mate[open.back()] = p;
      open.pop_back();
    } else if (db[p] != '.') return "a structure holds ( ) . only";
  }
  return open.empty() ? "" : "unbalanced structure";
}

// Appends the stems -- the maximal runs of directly nested pairs -- by increasing 5' end: (i, d, len) of the outermost pair.
inline void structure_stems(const int32_t* mate, int L, std::vector<int32_t>* s_i, std::vector<int32_t>* s_d, std::vector<int32_t>* s_len) {
  for (int p = 0; p < L; ++p) {
    const int r = mate[p];
    if (r < p || (p > 0 && r + 1 < L && mate[p - 1] == r + 1)) continue;   // (no 5' base, or not the outermost pair of its stem)
    int len = 1;
    while (p + len < r - len && mate[p + len] == r - len) ++len;
    s_i->push_back(p); s_d->push_back(r - p + 1); s_len->push_back(len);
  }
}

// Appends the loop every pair closes, by increasing 5' end: (type, i, d, k, l), the type 1 .. 5 for H S B I M (LoopType of
// loop_rules.h), (k, l) the cell of the inner pair -- l exclusive -- of a bulge or an interior loop and (-1, -1) otherwise.
inline void structure_loops(const int32_t* mate, int L, std::vector<int32_t>* s_type, std::vector<int32_t>* s_i, std::vector<int32_t>* s_d,
                            std::vector<int32_t>* s_k, std::vector<int32_t>* s_l) {
  for (int p = 0; p < L; ++p) {
    const int r = mate[p];
    if (r < p) continue;
    int inner = 0, k = -1, l = -1;
    for (int u = p + 1; u < r;) {
      if (mate[u] > u) { if (inner++ == 0) { k = u; l = mate[u]; } u = mate[u] + 1; }
      else ++u;
    }
    int type = 1;
    if (inner > 1) type = 5;
    else if (inner == 1) type = (k == p + 1 && l == r - 1) ? 2 : ((k == p + 1) != (l == r - 1)) ? 3 : 4;
    const bool twol = type == 3 || type == 4;
    s_type->push_back(type); s_i->push_back(p); s_d->push_back(r - p + 1);
    s_k->push_back(twol ? k : -1); s_l->push_back(twol ? l + 1 : -1);
  }
}

}  // namespace elemdp
