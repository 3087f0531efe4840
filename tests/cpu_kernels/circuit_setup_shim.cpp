// CPU build of the launch plan of the circuit setup (nim_groth16_amd/csrc/circuit_setup_plan.hpp), for
// tests/test_circuit_setup_cpu.py: the same functions the host layer and the kernels call.
#include <vector>

#include "../../nim_groth16_amd/csrc/circuit_setup_plan.hpp"

using namespace g16;

extern "C" {

uint32_t shim_cs_block() { return CS_BLOCK; }
uint32_t shim_cs_nbins() { return NBINS; }
uint32_t shim_bin_glog(uint32_t b) { return bin_glog(b); }
uint32_t shim_bin_of(uint32_t len) { return bin_of(len); }
uint32_t shim_pintt_max_log2() { return PINTT_MAX_LOG2; }
uint32_t shim_pintt_stages(uint32_t log2n) { return pintt_stages(log2n); }
uint32_t shim_pintt_butterflies(uint32_t log2n) { return pintt_butterflies(log2n); }
uint32_t shim_pintt_stage_grid(uint32_t log2n) { return pintt_stage_grid(log2n); }
uint32_t shim_pintt_twiddles(uint32_t log2n) { return pintt_twiddles(log2n); }
uint32_t shim_pintt_rev(uint32_t log2n, uint32_t i) { return pintt_rev(log2n, i); }

// every butterfly of stage s: lo[t], hi[t], tw[t], t < pintt_butterflies(log2n)
void shim_pintt_stage(uint32_t log2n, uint32_t s, uint32_t* lo, uint32_t* hi, uint32_t* tw) {
  for (uint32_t t = 0; t < pintt_butterflies(log2n); ++t) {
    const PinttPair p = pintt_pair(log2n, s, t);
    lo[t] = p.lo, hi[t] = p.hi, tw[t] = p.tw;
  }
}

// Stage s as the grid runs it -- lanes t = block * CS_BLOCK + lane, those at or beyond the butterfly count idle: how
// many times is each element touched, and is every pair 2^s apart with the twiddle of its position?  0 = every element
// exactly once and every twiddle right; else 1 + the first offending lane.
uint64_t shim_pintt_check_stage(uint32_t log2n, uint32_t s) {
  const uint64_t n = uint64_t(1) << log2n;
  std::vector<unsigned char> seen(n, 0);
  const uint64_t lanes = (uint64_t)pintt_stage_grid(log2n) * CS_BLOCK;
  if (lanes < pintt_butterflies(log2n) || lanes >= (uint64_t)pintt_butterflies(log2n) + CS_BLOCK) return ~uint64_t(0);
  for (uint64_t t = 0; t < lanes; ++t) {
    if (t >= pintt_butterflies(log2n)) continue;
    const PinttPair p = pintt_pair(log2n, s, (uint32_t)t);
    if (p.hi >= n || p.hi != p.lo + (1u << s) || seen[p.lo] || seen[p.hi]) return 1 + t;
    // position j of the lower element inside its block of 2^(s+1): the twiddle is omega_n^-(j n / 2^(s+1))
    const uint64_t j = p.lo & ((uint64_t(2) << s) - 1);
    if (j >= (uint64_t(1) << s) || p.tw != j * (n >> (s + 1)) || p.tw >= pintt_twiddles(log2n)) return 1 + t;
    seen[p.lo] = seen[p.hi] = 1;
  }
  for (uint64_t i = 0; i < n; ++i)
    if (!seen[i]) return 1 + lanes + i;
  return 0;
}

// out = first[NBINS] | count[NBINS] | grid[NBINS]
void shim_cs_sum_plan(const uint32_t* len, uint32_t nwires, uint32_t* wires, uint32_t* out) {
  const CsSumPlan p = cs_sum_plan(len, nwires, wires);
  for (int b = 0; b < NBINS; ++b) out[b] = p.first[b], out[NBINS + b] = p.count[b], out[2 * NBINS + b] = p.grid[b];
}

}  // extern "C"
