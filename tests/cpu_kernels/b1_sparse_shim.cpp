// Test-only: the sparse run of the B1 differences -- when a key takes it (key_plan.hpp) and the hit list its kernel builds
// from a live wire's scalar (msm_hit_list over msm_digit_walk, msm_params.hpp: the digit walk of the sort itself) --
// compiled with g++.  Not part of the product library.
#include "../../nim_groth16_amd/csrc/key_plan.hpp"
#include "../../nim_groth16_amd/csrc/msm_plan.hpp"
using namespace g16;

extern "C" {
uint64_t shim_b1_sparse_max() { return B1_SPARSE_MAX; }
int shim_b1_sparse_run(uint64_t live_delta) { return b1_sparse_run((size_t)live_delta) ? 1 : 0; }

// The launch parameters of a set of n points registered with window c, `mtab` multiplier tables and tables at `stride`
// (msm_params over msm_table_cfg), and the hits of pair i with the canonical scalar `scalar` (8 words, least significant
// first): out = nwin (slot, entry) pairs, geom = {nwin, nbuckets, mtab, tstride}.  -> the number of hits
uint32_t shim_hit_list(const uint32_t scalar[8], uint32_t i, uint64_t n, uint32_t c, uint32_t mtab, uint32_t stride,
                       uint32_t* out, uint32_t geom[4]) {
  G16Env env;
  const MsmParams P = msm_params((size_t)n, 0, msm_table_cfg(c, mtab, stride), env);
  geom[0] = P.nwin, geom[1] = P.nbuckets, geom[2] = P.mtab, geom[3] = P.tstride;
  uint32_t s[8];
  for (int j = 0; j < 8; ++j) s[j] = scalar[j];
  MsmHit hits[256];
  const uint32_t k = msm_hit_list(s, i, P, hits);
  for (uint32_t j = 0; j < k; ++j) out[2 * j] = hits[j].slot, out[2 * j + 1] = hits[j].entry;
  return k;
}
}
