// Kernels of the key audit (audit.hip): one pass per array of a proving key that an untrusted party supplied.
//
// Per element, three checks in this precedence -- an element that fails one is counted there and not examined further:
//   0  canonical   every Fp limb pattern is < p (the field arithmetic would silently reduce a larger one, so an alias
//                  of a valid point would pass everything below)
//   1  on curve    y^2 = x^3 + b, (0,0) = infinity passes
//   2  order r     G2 only: [r]Q == infinity, by the definition -- no endomorphism shortcut.  G1 has cofactor 1.
// The order-r test is the one hot path: one lane per point, but the multiplier is the constant r, so the lanes walk the
// fixed double / add schedule of subgroup_plan.hpp and never branch on a scalar bit.  What diverges inside a wave: a
// lane that failed check 0 or 1 or holds infinity (it skips the ladder), and the exceptional paths of the complete
// additions (G2::dbl / G2::madd; a point of small order reaches them, an honest point only in the last addition,
// (r -+ 1) Q +- Q, where the opposite-operands path is the main path).
#pragma once
#include "pairing.cuh"
#include "subgroup_plan.hpp"

namespace g16 {

static_assert((uint32_t)SUBGROUP_R[0] == FrParams::P0 && (uint32_t)(SUBGROUP_R[0] >> 32) == FrParams::P1 &&
                  (uint32_t)SUBGROUP_R[1] == FrParams::P2 && (uint32_t)(SUBGROUP_R[1] >> 32) == FrParams::P3 &&
                  (uint32_t)SUBGROUP_R[2] == FrParams::P4 && (uint32_t)(SUBGROUP_R[2] >> 32) == FrParams::P5 &&
                  (uint32_t)SUBGROUP_R[3] == FrParams::P6 && (uint32_t)(SUBGROUP_R[3] >> 32) == FrParams::P7,
              "subgroup_plan.hpp is the schedule of another number than Fr's modulus");

// per array and check: index of the first failing element (0xffffffff on entry = none) and how many fail
struct AuditCounts {
  uint32_t first_bad[3];
  uint32_t bad_count[3];
};

static __constant__ SubgroupPlan AUDIT_SUBGROUP_PLAN = make_subgroup_plan();

// [r]Q == infinity for Q on the twist, Q != infinity: the schedule of subgroup_plan.hpp on the complete additions.
// The lane's point waits in LDS between the additions (`park`: AUDIT_Q_WORDS x blockDim.x words, word-major, so a wave
// reads consecutive banks): held in registers beside the accumulator and the temporaries of a mixed addition it
// pushed the loop over 256 VGPRs.
constexpr int AUDIT_Q_WORDS = sizeof(g2_aff) / 4;
static __device__ __forceinline__ bool audit_order_r(const g2_aff& q, uint32_t* park) {
  {
    const uint32_t* w = reinterpret_cast<const uint32_t*>(&q);
#pragma unroll
    for (int k = 0; k < AUDIT_Q_WORDS; ++k) park[k * blockDim.x + threadIdx.x] = w[k];
  }
  g2_acc acc{q.x, q.y, Fp2::one(), Fp2::one()};   // the leading digit
  const int nsteps = AUDIT_SUBGROUP_PLAN.nsteps;
#pragma unroll 1
  for (int s = 0; s < nsteps; ++s) {
    const SubgroupStep st = AUDIT_SUBGROUP_PLAN.step[s];   // wave-uniform: scalar loads, scalar branches
#pragma unroll 1
    for (int b = 0; b < st.dbls; ++b) acc = G2::dbl(acc);
    __asm__ volatile("" ::: "memory");   // the reload below stays inside the loop
    g2_aff a;
    {
      uint32_t* w = reinterpret_cast<uint32_t*>(&a);
#pragma unroll
      for (int k = 0; k < AUDIT_Q_WORDS; ++k) w[k] = park[k * blockDim.x + threadIdx.x];
    }
    if (st.digit < 0) a.y = Fp2::neg(a.y);
    G2::madd(acc, a);
  }
  return G2::is_inf(acc);
}

static __device__ __forceinline__ bool audit_canonical(const g1_aff& p) {
  return Fp::is_canonical(p.x) && Fp::is_canonical(p.y);
}
static __device__ __forceinline__ bool audit_canonical(const g2_aff& p) {
  return Fp::is_canonical(p.x.c0) && Fp::is_canonical(p.x.c1) && Fp::is_canonical(p.y.c0) && Fp::is_canonical(p.y.c1);
}

// The checks of one element: -1 = passes, else the check it fails.  ORDER = 0: checks 0 and 1 only (G1),
// ORDER = 1: the fixed schedule, ORDER = 2: the caller's ladder `gen` (tools/ubench_subgroup.hip measures the generic
// double-and-add of pairing.hip beside the fixed schedule through this hook; the library never instantiates it)
template <class C, int ORDER, class Gen>
static __device__ __forceinline__ int audit_element(const typename C::Aff& p, const typename C::E& b, uint32_t* park,
                                                    Gen gen) {
  using F = typename C::Field;
  if (!audit_canonical(p)) return 0;
  if (C::is_inf(p)) return -1;
  if (!F::eq(F::sqr(p.y), F::add(F::mul(F::sqr(p.x), p.x), b))) return 1;
  if constexpr (ORDER == 1) {
    if (!audit_order_r(p, park)) return 2;
  } else if constexpr (ORDER == 2) {
    if (!gen(p)) return 2;
  }
  return -1;
}
struct AuditNoLadder {
  template <class A>
  __device__ bool operator()(const A&) const { return true; }
};

// Occupancy.  The ladder keeps the accumulator (4 Fp2 = 64 VGPRs) and the temporaries of one complete mixed addition
// live; the point itself is parked in LDS (audit_order_r).  G2: hipcc reports 241 VGPRs and no scratch under
// __launch_bounds__(256, 2): 2 waves per SIMD, the occupancy of the G2 bucket-accumulation kernel, with two
// workgroups of 32 KiB LDS per CU.  (3 waves, 168 VGPRs, spills 372 bytes per lane, 4 waves 608; without the LDS
// parking the loop needed 257 registers: one wave per SIMD.)  The kernel is VALU-bound.
// G1 (checks 0 and 1 only) is a memory-bound scan: 44 VGPRs.
constexpr int AUDIT_BLOCK = 256;
constexpr int AUDIT_WAVES = 2;   // per SIMD

template <class C, int ORDER>
__global__ void __launch_bounds__(AUDIT_BLOCK, AUDIT_WAVES) audit_points(const typename C::Aff* __restrict__ pts, uint32_t n,
                                                            typename C::E b, AuditCounts* __restrict__ out) {
  const uint32_t i = blockIdx.x * AUDIT_BLOCK + threadIdx.x;
  if (i >= n) return;
  extern __shared__ uint32_t park[];   // ORDER == 1: AUDIT_Q_WORDS * AUDIT_BLOCK words; else none
  const typename C::Aff p = pts[i];
  const int bad = audit_element<C, ORDER>(p, b, park, AuditNoLadder{});
  if (bad < 0) return;
  atomicMin(&out->first_bad[bad], i);
  atomicAdd(&out->bad_count[bad], 1u);
}

// Canonical scan of the coefficient values of a key: record e holds its 32-byte value at word off_w of stride_w
// 32-bit words (g16_coeff: 12 / 4; section 4 of a .zkey after its count: 11 / 3).  Both forms must be < r: a Montgomery
// value, and the doubly-Montgomery integer of the file.
__global__ void __launch_bounds__(256) audit_coeffs(const uint32_t* __restrict__ words, uint32_t count,
                                                    uint32_t stride_w, uint32_t off_w, AuditCounts* __restrict__ out) {
  const uint32_t e = blockIdx.x * 256 + threadIdx.x;
  if (e >= count) return;
  const uint32_t* w = words + (size_t)e * stride_w + off_w;
  u256 v;
#pragma unroll
  for (int k = 0; k < 8; ++k) v.v[k] = w[k];
  if (Fr::is_canonical(v)) return;
  atomicMin(&out->first_bad[0], e);
  atomicAdd(&out->bad_count[0], 1u);
}

// result[j] = ( e(a[j], gen2) * e(-gen1, b[j]) == 1 ): a[j] and b[j] are the same multiple of the two generators.
// One workgroup per relation; lanes 0 and 1 run the two Miller loops, lane 0 the final exponentiation.
__global__ void __launch_bounds__(64) audit_relation(const g1_aff* __restrict__ a, const g2_aff* __restrict__ b,
                                                     g1_aff neg_gen1, g2_aff gen2, int32_t* __restrict__ result) {
  __shared__ fp12_t sh[2];
  const uint32_t j = blockIdx.x, lane = threadIdx.x;
  if (lane < 2) {
    fp12_t f;
    const g1_aff P = lane ? neg_gen1 : a[j];
    const g2_aff Q = lane ? b[j] : gen2;
    Pairing::miller(f, P, Q);
    sh[lane] = f;
  }
  __syncthreads();
  if (lane) return;
  fp12_t t, f;
  const fp12_t m0 = sh[0], m1 = sh[1];
  Pairing::mul(t, m0, m1);
  Pairing::final_exp(f, t);
  result[j] = Pairing::is_one(f) ? 1 : 0;
}

}  // namespace g16
