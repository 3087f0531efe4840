// witness_plan.hpp on the CPU (tests/test_witness_check_cpu.py): the ordered list of failing constraints out of a bitmap.
// stdin, one case per line:  <constraints> <lanes> <count> <index> ...   (the set bits)
// stdout, one line per case:  <words read> <list[0]> ... <list[15]>       (4294967295 = none)
#include <cstdio>
#include <vector>

#include "../../nim_groth16_amd/csrc/witness_plan.hpp"

int main() {
  unsigned long long ncons, lanes, count;
  while (scanf("%llu %llu %llu", &ncons, &lanes, &count) == 3) {
    std::vector<uint64_t> bitmap(g16::witness_words(ncons) + 1, 0);   // + 1: an empty bitmap still has an address
    for (unsigned long long k = 0; k < count; ++k) {
      unsigned long long i;
      if (scanf("%llu", &i) != 1 || i >= ncons) return 2;
      bitmap[i / 64] |= uint64_t(1) << (i % 64);
    }
    uint32_t list[g16::WITNESS_LIST];
    const size_t read = g16::witness_select(bitmap.data(), g16::witness_words(ncons), (uint32_t)lanes, list);
    printf("%zu", read);
    for (uint32_t k = 0; k < g16::WITNESS_LIST; ++k) printf(" %u", list[k]);
    printf("\n");
  }
  return 0;
}
