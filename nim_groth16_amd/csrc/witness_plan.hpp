// The ordered list of a witness report (include/g16hip.h, "witness check"): the WITNESS_LIST smallest failing constraint
// indices out of a bitmap of one bit per constraint, as a pure function.  Plain C++17 and no HIP header: the list kernel
// (witness_check.hip) and the CPU test (tests/cpu_kernels/witness_plan_main.cpp) run the same two functions.
//
// The bitmap is written by the row kernel, one 64-bit word per wave (bit l of word j = constraint 64 j + l fails), so it
// is complete before the list is made and the list does not depend on the order in which the waves ran.  The list kernel
// is ONE workgroup that walks the words in ascending order, WITNESS_LANES words per trip:
//   * lane t holds word base + t and counts its bits;
//   * an exclusive prefix sum over the lanes tells lane t how many failing constraints lie before its word (`before`);
//   * witness_take writes the lane's bits to the slots before, before + 1, ... while they are < WITNESS_LIST;
//   * the trip's total is added to `found`, and the walk stops once found >= WITNESS_LIST: a witness with many failures
//     is settled by the first words, a clean one never starts the walk (bad_count == 0).
// witness_select is the same walk on the host, trip by trip, with the prefix sum as a loop.
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define WITNESS_HD __host__ __device__
#else
#define WITNESS_HD
#endif

namespace g16 {

constexpr uint32_t WITNESS_LIST = 16;      // G16_WITNESS_LIST
constexpr uint32_t WITNESS_BLOCK = 256;    // lanes of the row kernel: four waves, four bitmap words per workgroup
constexpr uint32_t WITNESS_LANES = 256;    // lanes of the list kernel = bitmap words per trip
constexpr uint32_t WITNESS_NONE = 0xffffffffu;

WITNESS_HD inline uint32_t witness_popcount(uint64_t w) {
  uint32_t c = 0;
  for (; w; w &= w - 1) ++c;
  return c;
}

inline size_t witness_words(size_t nconstraints) { return (nconstraints + 63) / 64; }

// the set bits of `word` (bitmap word `word_index`), ascending, into list[before], list[before + 1], ... while the slot
// exists; `before` = the set bits of every earlier word.  Returns the number of slots written.
WITNESS_HD inline uint32_t witness_take(uint64_t word, uint32_t word_index, uint32_t before, uint32_t* list) {
  uint32_t written = 0;
  for (uint32_t bit = 0; word && before + written < WITNESS_LIST; ++bit, word >>= 1)
    if (word & 1) list[before + written++] = 64u * word_index + bit;
  return written;
}

// list[0 .. WITNESS_LIST): the smallest set bits of the bitmap, ascending, the rest WITNESS_NONE.  `lanes` words per trip.
// Returns the number of words it read (the early exit is part of what the test holds).
inline size_t witness_select(const uint64_t* bitmap, size_t nwords, uint32_t lanes, uint32_t* list) {
  for (uint32_t k = 0; k < WITNESS_LIST; ++k) list[k] = WITNESS_NONE;
  uint32_t found = 0;
  size_t base = 0;
  for (; base < nwords && found < WITNESS_LIST; base += lanes) {
    uint32_t before = found;
    for (uint32_t t = 0; t < lanes && base + t < nwords; ++t) {
      const uint64_t w = bitmap[base + t];
      if (before < WITNESS_LIST) witness_take(w, (uint32_t)(base + t), before, list);
      before += witness_popcount(w);
    }
    found = before;
  }
  return base < nwords ? base : nwords;
}

}  // namespace g16
