// CPU build of the per-point scaling (nim_groth16_amd/csrc/scale_each.cuh) for tests/test_phase1_cpu.py: the split a lane
// makes of its own scalar and the lane arithmetic that walks it, the same functions the kernel calls.
#include <cstring>

#include "../../nim_groth16_amd/csrc/scale_each.cuh"

using namespace g16;

// The launch of scale_each<G1 / G2> lane by lane: every workgroup of the grid over n points, every lane of it, the parking
// slots in an array.  scalars: n x 32 bytes, canonical.  In place (out == pts) as the library calls it.
template <class C>
static void scale_each_points(const void* pts, uint64_t n, const void* scalars, uint32_t mont, void* out) {
  typename C::E park[(SCALE_GROUP - 1) * 3];
  const uint64_t grid = (n + SCALE_TILE - 1) / SCALE_TILE;
  for (uint64_t blk = 0; blk < grid; ++blk)
    for (uint64_t lane = 0; lane < SCALE_BLOCK; ++lane)
      scale_each_lane<C>((const typename C::Aff*)pts, (const u256*)scalars, mont, n, blk * SCALE_TILE + lane, SCALE_BLOCK,
                         [&](int s) -> typename C::E& { return park[s]; }, (typename C::Aff*)out);
}

extern "C" {

// count scalars (32 bytes each, standard form, canonical) -> per scalar halves[4 i ..] = |k1| (2 x 64 bits) | |k2|, signs[i]
// bit 0: k1 < 0, bit 1: k2 < 0, bit 2: a magnitude does not fit 128 bits
void shim_each_split(const void* scalars, uint64_t count, uint64_t* halves, uint32_t* signs) {
  for (uint64_t i = 0; i < count; ++i) {
    u256 k;
    memcpy(&k, (const char*)scalars + 32 * i, 32);
    const EachSplit s = scale_each_split(k);
    halves[4 * i] = s.k1[0] | (uint64_t)s.k1[1] << 32, halves[4 * i + 1] = s.k1[2] | (uint64_t)s.k1[3] << 32;
    halves[4 * i + 2] = s.k2[0] | (uint64_t)s.k2[1] << 32, halves[4 * i + 3] = s.k2[2] | (uint64_t)s.k2[3] << 32;
    signs[i] = (s.neg1 ? 1u : 0u) | (s.neg2 ? 2u : 0u) | (s.ok ? 0u : 4u);
  }
}

void shim_each_points_g1(const void* pts, uint64_t n, const void* scalars, uint32_t mont, void* out) {
  scale_each_points<G1>(pts, n, scalars, mont, out);
}
void shim_each_points_g2(const void* pts, uint64_t n, const void* scalars, uint32_t mont, void* out) {
  scale_each_points<G2>(pts, n, scalars, mont, out);
}

}  // extern "C"
