// Test-only driver of the structure parser (rnaelem_amd/csrc/structure_rules.h): a stand-alone program, built by
// tests/test_structure_rules_cpu.py with the address and undefined-behaviour sanitizers.  Reads one dot-bracket string per line
// from stdin (an empty line is the empty string) and answers one line per string:
//   ok S i d len .. L type i d k l ..      the stems, then the loops, every column as structure_stems / structure_loops append it
//   error <what structure_mates returned>
#include <cstdio>
#include <iostream>
#include <string>
#include <vector>

#include "../rnaelem_amd/csrc/structure_rules.h"

using namespace elemdp;

int main() {
  std::string db;
  while (std::getline(std::cin, db)) {
    const int L = (int)db.size();
    std::vector<int32_t> mate((size_t)L), s_i, s_d, s_len, l_t, l_i, l_d, l_k, l_l;
    const char* err = structure_mates(db.data(), L, mate.data());
    if (*err) { printf("error %s\n", err); continue; }
    structure_stems(mate.data(), L, &s_i, &s_d, &s_len);
    structure_loops(mate.data(), L, &l_t, &l_i, &l_d, &l_k, &l_l);
    printf("ok S");
    for (size_t k = 0; k < s_i.size(); ++k) printf(" %d %d %d", s_i[k], s_d[k], s_len[k]);
    printf(" L");
    for (size_t k = 0; k < l_i.size(); ++k) printf(" %d %d %d %d %d", l_t[k], l_i[k], l_d[k], l_k[k], l_l[k]);
    printf("\n");
  }
  return 0;
}
