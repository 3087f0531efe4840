// Launch shapes of the circuit setup (circuit_setup.cuh / circuit_setup.hip) as pure functions, shared by host code, by
// the kernels and by the CPU test shim (plain C++: the shim is built with g++).
//
// Group inverse NTT of 2^log2n points: the input is loaded in bit-reversed order (one lane per element, which also
// applies the element's scalar: 1/n, or the coset factor of the snarkjs H points), then log2n radix-2 stages run in
// place over global memory, one launch per stage, one lane per butterfly, natural order out.  Stage s pairs elements
// 2^s apart; butterfly t of it multiplies its upper element by omega^-(j 2^(log2n-1-s)), j = t mod 2^s -- twiddle
// index 0 is the factor one and is not multiplied.
//
// Sparse matrix x point vector: the terms of a wire lie together (the host sorts the entries by wire); the sum pass
// gives a wire the lanes of its bin of spmv_params.hpp -- one lane up to 4 terms, 2^g lanes up to 4 * 2^g, 64 lanes in
// strided trips beyond -- and is launched once per bin that holds a wire.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "spmv_params.hpp"

namespace g16 {

constexpr uint32_t CS_BLOCK = 64;          // lanes per workgroup of every kernel of circuit_setup.cuh: one wave
constexpr uint32_t PINTT_MAX_LOG2 = 24;    // g16_points_intt_*: 2^23 twiddles of 32 B, a G2 working vector of 4 GB

static_assert((1u << bin_glog(NBINS - 1)) <= CS_BLOCK, "the lanes of a wire sit in one workgroup");

G16_SPMV_HD uint32_t cs_grid(uint64_t lanes) { return (uint32_t)((lanes + CS_BLOCK - 1) / CS_BLOCK); }

// ---- group inverse NTT ---------------------------------------------------------------------------------------------------
G16_SPMV_HD uint32_t pintt_stages(uint32_t log2n) { return log2n; }
G16_SPMV_HD uint32_t pintt_butterflies(uint32_t log2n) { return log2n ? 1u << (log2n - 1) : 0u; }
G16_SPMV_HD uint32_t pintt_stage_grid(uint32_t log2n) { return cs_grid(pintt_butterflies(log2n)); }
G16_SPMV_HD uint32_t pintt_twiddles(uint32_t log2n) { return pintt_butterflies(log2n); }   // omega^-k, k < n/2
// where element i of the input goes: the bit reversal of i over log2n bits
G16_SPMV_HD uint32_t pintt_rev(uint32_t log2n, uint32_t i) {
  uint32_t r = 0;
  for (uint32_t b = 0; b < log2n; ++b) r |= ((i >> b) & 1u) << (log2n - 1 - b);
  return r;
}
struct PinttPair {
  uint32_t lo, hi, tw;   // the two elements of the butterfly and its twiddle index
};
G16_SPMV_HD PinttPair pintt_pair(uint32_t log2n, uint32_t s, uint32_t t) {
  const uint32_t j = t & ((1u << s) - 1u);
  const uint32_t lo = ((t >> s) << (s + 1)) | j;
  return PinttPair{lo, lo + (1u << s), j << (log2n - 1 - s)};
}

// ---- sum pass --------------------------------------------------------------------------------------------------------------
struct CsSumPlan {
  uint32_t first[NBINS], count[NBINS], grid[NBINS];   // the wires of bin b: wires[first[b] .. first[b] + count[b])
};
// len[w] = terms of wire w; wires (nwires slots) receives the wires grouped by bin, in wire order inside a bin
inline CsSumPlan cs_sum_plan(const uint32_t* len, uint32_t nwires, uint32_t* wires) {
  CsSumPlan p{};
  for (uint32_t w = 0; w < nwires; ++w) ++p.count[bin_of(len[w])];
  uint32_t at = 0, cursor[NBINS];
  for (int b = 0; b < NBINS; ++b) {
    p.first[b] = cursor[b] = at;
    at += p.count[b];
    p.grid[b] = cs_grid((uint64_t)p.count[b] << bin_glog(b));
  }
  for (uint32_t w = 0; w < nwires; ++w) wires[cursor[bin_of(len[w])]++] = w;
  return p;
}

}  // namespace g16
