// CPU build of the uniform-scalar schedule (nim_groth16_amd/csrc/scale_plan.hpp) and of the lane arithmetic that walks it
// (scale.cuh), for tests/test_phase2_cpu.py: the same functions the host layer and the kernel call.
#include <cstring>

#include "../../nim_groth16_amd/csrc/scale.cuh"

using namespace g16;

// The launch of scale_uniform<G1 / G2> lane by lane: every workgroup of the grid over n points, every lane of it, the
// parking slots in an array.  k: 32 bytes, standard form, canonical.  In place (out == pts) as the library calls it.
template <class C>
static void scale_points(const void* pts, uint64_t n, const uint64_t* k, void* out) {
  U256 kk;
  memcpy(kk.v, k, 32);
  const ScalePlan plan = make_scale_plan(kk);
  ScaleArgs args;
  args.steps = reinterpret_cast<const uint32_t*>(plan.step);
  args.nsteps = (uint32_t)plan.nsteps, args.tail_dbls = (uint32_t)plan.tail_dbls;
  memcpy(args.k.v, k, 32);
  typename C::E park[(SCALE_GROUP - 1) * 3];
  const uint64_t grid = (n + SCALE_TILE - 1) / SCALE_TILE;
  for (uint64_t blk = 0; blk < grid; ++blk)
    for (uint64_t lane = 0; lane < SCALE_BLOCK; ++lane)
      scale_lane<C>((const typename C::Aff*)pts, n, blk * SCALE_TILE + lane, SCALE_BLOCK, args,
                    [&](int s) -> typename C::E& { return park[s]; }, (typename C::Aff*)out);
}

extern "C" {

uint32_t shim_scale_block() { return SCALE_BLOCK; }
uint32_t shim_scale_group() { return SCALE_GROUP; }
uint32_t shim_scale_max_steps() { return ScalePlan::MAX_STEPS; }
// out = r | lambda | beta, 32 bytes each, little-endian, standard form
void shim_scale_consts(uint64_t* out) {
  memcpy(out, SCALE_R.v, 32);
  memcpy(out + 4, SCALE_LAMBDA.v, 32);
  memcpy(out + 8, SCALE_BETA.v, 32);
}

// halves[0..1] = |k1|, halves[2..3] = |k2| (little-endian 64-bit limbs); signs bit 0: k1 < 0, bit 1: k2 < 0.
// Returns 1 if the decomposition's own assertions hold.
int32_t shim_scale_split(const uint64_t* k, uint64_t* halves, uint32_t* signs) {
  U256 kk;
  memcpy(kk.v, k, 32);
  const ScaleSplit s = scale_split(kk);
  halves[0] = (uint64_t)s.k1, halves[1] = (uint64_t)(s.k1 >> 64);
  halves[2] = (uint64_t)s.k2, halves[3] = (uint64_t)(s.k2 >> 64);
  *signs = (s.neg1 ? 1u : 0u) | (s.neg2 ? 2u : 0u);
  return s.ok ? 1 : 0;
}

// steps: nsteps x {dbls, entry, sign, 0} bytes (room for shim_scale_max_steps()); info = nsteps, ndbl, tail_dbls;
// value = what the independent checker evaluates the plan to.  Returns 1 if the decomposition's assertions hold.
int32_t shim_scale_plan(const uint64_t* k, uint8_t* steps, int32_t* info, uint64_t* value) {
  U256 kk;
  memcpy(kk.v, k, 32);
  bool ok = false;
  const ScalePlan p = make_scale_plan(kk, &ok);
  memcpy(steps, p.step, sizeof(ScaleStep) * (size_t)p.nsteps);
  info[0] = p.nsteps, info[1] = p.ndbl, info[2] = p.tail_dbls;
  const U256 v = scale_plan_value(p);
  memcpy(value, v.v, 32);
  return ok ? 1 : 0;
}

void shim_scale_points_g1(const void* pts, uint64_t n, const uint64_t* k, void* out) { scale_points<G1>(pts, n, k, out); }
void shim_scale_points_g2(const void* pts, uint64_t n, const uint64_t* k, void* out) { scale_points<G2>(pts, n, k, out); }

}  // extern "C"
