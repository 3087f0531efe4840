// Test-only: the layout rules of a resident proving key (key_plan.hpp) compiled with g++.  Not part of the product
// library.
#include "../../nim_groth16_amd/csrc/key_plan.hpp"
using namespace g16;

extern "C" {
// the index range of shard `index` of `count` over N indices
void shim_shard_range(uint64_t N, uint32_t index, uint32_t count, uint64_t out[2]) {
  const KeyRange r = shard_range((size_t)N, index, count);
  out[0] = r.lo, out[1] = r.hi;
}
// C1 slots of the wire range [lo, hi) that are the padding of the public wires 0 .. npubs
uint64_t shim_c1_padding(uint64_t lo, uint64_t hi, uint32_t npubs) {
  return c1_padding(KeyRange{(size_t)lo, (size_t)hi}, npubs);
}
// where liveB / deadB come from (LiveSource), and -- once the dead count is known -- whether the bitmap is kept, under
// G16_INF_COMPACT = pct
int shim_live_b_source(int form, uint64_t nw, int b1_bitmap, int b2_bitmap) {
  return (int)live_b_source(form, (size_t)nw, b1_bitmap != 0, b2_bitmap != 0);
}
int shim_live_b_kept(int source, uint64_t dead, uint64_t nw, int pct) {
  G16Env env;
  env.inf_compact_pct = pct;
  return live_b_kept((LiveSource)source, (size_t)dead, (size_t)nw, env) ? 1 : 0;
}
}
