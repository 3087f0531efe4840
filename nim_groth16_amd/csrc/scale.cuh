// out[i] = k * P[i] for ONE scalar k and an array of points, affine in and affine out (include/g16hip.h, "scaling an
// array of points"; host layer: scale.hip; the schedule: scale_plan.hpp).  Instantiated per curve in scale_g1.hip /
// scale_g2.hip.
//
// G1.  The lane never sees k: it walks the joint-sparse-form schedule of (k1, k2), k = k1 + k2 lambda, that the host
// uploaded -- ~127 doublings and ~64 additions in place of 254 and ~127.  Its table is P, phi P, P + phi P, P - phi P:
//   phi P = (beta x, y) and P + phi P = -phi^2 P = (beta^2 x, -y) cost one multiplication each;
//   P - phi P is a real addition, with denominator t = (beta - 1) x.  Rather than invert t per lane, or keep that entry
//   in XYZZ and pay the full addition (12M + 2S against 8M + 2S) in a quarter of the steps, the whole ladder runs on
//   the isomorphic curve E': y^2 = x^3 + b t^6 through (x, y) -> (t^2 x, t^3 y).  There P - phi P is affine with no
//   division (its XYZZ form on E has ZZ = t^2, ZZZ = t^3), the other three entries cost one multiplication more each,
//   every addition is the mixed one, and the way back is acc.zz *= t^2, acc.zzz *= t^3.  The formulas of ec.cuh for
//   a = 0 never read b, so dbl / madd ARE the complete additions of E'.  The table is six field elements (x', beta x',
//   beta^2 x', y', and the difference's two) in registers; the entry and sign of a step are wave-uniform selects.
// G2 has no endomorphism here: the bit ladder of scalar_mul.cuh over k.
//
// Affine output.  A lane handles SCALE_GROUP points one after the other and inverts once for all of them (Montgomery's
// trick over the lane's own points: across the lanes of a wave a shared inversion saves no time, the wave pays for
// one inversion whether one lane runs it or all).  Point j leaves a = X zzz c, b = Y zz c, d = zz zzz, c = the product
// of the d before it, parked in LDS (the last one stays in registers); then x = a / (c d), walking back.  A point at
// infinity (zz zzz = 0) enters the product as d = 1 with a = b = 0: it comes out as (0,0) and the group never sees a
// zero.  Nothing in XYZZ form goes through global memory.
// The arithmetic of a lane (scale_ladder, scale_lane) is plain FF_HD code: tests/cpu_kernels/scale_plan_shim.cpp runs it
// with g++ against the oracle; only the kernel and its launcher need HIP.
#pragma once
#if defined(__HIPCC__)
#include "g16_internal.hpp"
#endif
#include "scalar_mul.cuh"
#include "scale_plan.hpp"

namespace g16 {

// beta, beta^2 and beta - 1 in Fp, Montgomery form (SCALE_BETA of scale_plan.hpp; tests/test_phase2_cpu.py re-derives
// them from the standard form)
FF_HD u256 scale_beta() {
  return u256{{0xd782e155u, 0x71930c11u, 0xffbe3323u, 0xa6bb947cu, 0xd4741444u, 0xaa303344u, 0x26594943u, 0x2c3b3f0du}};
}
FF_HD u256 scale_beta_sqr() {
  return u256{{0x13e80b9cu, 0x3350c88eu, 0xdb5e56b9u, 0x7dce557cu, 0xb615564au, 0x6001b4b8u, 0x020217e0u, 0x2682e617u}};
}
FF_HD u256 scale_beta_minus_one() {
  return u256{{0x11f3d3b8u, 0x9e35c884u, 0x09f727e5u, 0x9c42a954u, 0x5bface18u, 0x43c18fd5u, 0x8c516a14u, 0x1e30c74bu}};
}

struct ScaleArgs {
  const uint32_t* steps;   // G1: the uploaded schedule
  uint32_t nsteps, tail_dbls;
  u256 k;                  // G2: the scalar, standard form
};

// k * p on G1 by the schedule; p on the curve or (0,0)
FF_HD g1_acc scale_ladder(const g1_aff& p, const ScaleArgs& a) {
  if (G1::is_inf(p)) return G1::acc_inf();
  // the table on E' (header): x0 = t^2 x, y0 = t^3 y
  u256 x0, x1, x2, y0, xd, yd;
  {
    const u256 t = Fp::mul(scale_beta_minus_one(), p.x);
    const u256 tt = Fp::sqr(t), ttt = Fp::mul(t, tt);
    x0 = Fp::mul(p.x, tt);
    y0 = Fp::mul(p.y, ttt);
    x1 = Fp::mul(scale_beta(), x0);
    x2 = Fp::mul(scale_beta_sqr(), x0);
    // P - phi P = P + (beta x, -y) by madd-2008-s from zz = zzz = 1: p = t, r = -2 y, qq = x tt = x0
    const u256 r = Fp::neg(Fp::dbl(p.y));
    xd = Fp::sub(Fp::sub(Fp::sqr(r), ttt), Fp::dbl(x0));
    yd = Fp::mulsub(r, Fp::sub(x0, xd), p.y, ttt);
  }
  g1_acc acc = G1::acc_inf();
#pragma unroll 1
  for (uint32_t s = 0; s < a.nsteps; ++s) {
    const uint32_t st = a.steps[s];   // wave-uniform: a scalar load
    const uint32_t dbls = st & 0xffu, entry = (st >> 8) & 0xffu;
    const bool minus = ((st >> 16) & 0x80u) != 0;   // sign = -1
#pragma unroll 1
    for (uint32_t b = 0; b < dbls; ++b) acc = G1::dbl(acc);
    g1_aff q;
    q.x = entry == SCALE_P ? x0 : entry == SCALE_PHI ? x1 : entry == SCALE_SUM ? x2 : xd;
    q.y = entry == SCALE_DIFF ? yd : y0;
    if (minus != (entry == SCALE_SUM)) q.y = Fp::neg(q.y);   // the table's sum entry is (x2, -y0)
    G1::madd(acc, q);
  }
#pragma unroll 1
  for (uint32_t b = 0; b < a.tail_dbls; ++b) acc = G1::dbl(acc);
  // back to E: zz *= t^2, zzz *= t^3 (infinity stays infinity: t != 0 for a point of the curve, which has no x = 0)
  const u256 t = Fp::mul(scale_beta_minus_one(), p.x);
  const u256 tt = Fp::sqr(t);
  acc.zz = Fp::mul(acc.zz, tt);
  acc.zzz = Fp::mul(acc.zzz, Fp::mul(t, tt));
  return acc;
}
FF_HD g2_acc scale_ladder(const g2_aff& p, const ScaleArgs& a) {
  return scalar_mul<G2>(p, a.k);
}

// The SCALE_GROUP points of one lane: index first + j * stride, j < SCALE_GROUP, those below n.  `ladder(i)`: the
// multiple of point i in XYZZ form, whatever scalar it takes (the one of scale_uniform here, the point's own in
// scale_each.cuh).  `park(k)`: the lane's k-th parking slot, k < 3 (SCALE_GROUP - 1) (LDS on the device).  In place
// (out == the array `ladder` reads) is fine: a lane writes only what it alone has read.
template <class C, class Ladder, class Park>
FF_HD void scale_group(uint64_t n, uint64_t first, uint64_t stride, Ladder ladder, Park park, typename C::Aff* out) {
  using F = typename C::Field;
  using E = typename C::E;
  E a = F::zero(), b = F::zero(), d = F::one(), c = F::one();
#pragma unroll 1
  for (int j = 0; j < SCALE_GROUP; ++j) {
    const uint64_t i = first + (uint64_t)j * stride;
    typename C::Acc acc = C::acc_inf();
    if (i < n) acc = ladder(i);
    d = F::mul(acc.zz, acc.zzz);
    if (F::is_zero(d)) {
      a = F::zero(), b = F::zero(), d = F::one();
    } else {
      a = F::mul(F::mul(acc.x, acc.zzz), c);
      b = F::mul(F::mul(acc.y, acc.zz), c);
    }
    if (j < SCALE_GROUP - 1) {
      park(3 * j) = a, park(3 * j + 1) = b, park(3 * j + 2) = d;
      c = F::mul(c, d);
    }
  }
  // c = d_0 .. d_(G-2); inv runs through 1 / (d_0 .. d_j), j = G-1 .. 0
  E inv = F::inv(F::mul(c, d));
#pragma unroll 1
  for (int j = SCALE_GROUP - 1; j >= 0; --j) {
    if (j < SCALE_GROUP - 1) a = park(3 * j), b = park(3 * j + 1), d = park(3 * j + 2);
    const uint64_t i = first + (uint64_t)j * stride;
    if (i < n) out[i] = typename C::Aff{F::mul(a, inv), F::mul(b, inv)};
    inv = F::mul(inv, d);
  }
}
template <class C, class Park>
FF_HD void scale_lane(const typename C::Aff* pts, uint64_t n, uint64_t first, uint64_t stride,
                      const ScaleArgs& args, Park park, typename C::Aff* out) {
  scale_group<C>(n, first, stride, [&](uint64_t i) { return scale_ladder(pts[i], args); }, park, out);
}

#if defined(__HIPCC__)
// One workgroup: SCALE_TILE consecutive points; lane t takes tile + j * SCALE_BLOCK + t, j < SCALE_GROUP.  No
// __restrict__: out may be pts.
template <class C>
__global__ void __launch_bounds__(SCALE_BLOCK) scale_uniform(const typename C::Aff* pts, uint32_t n, ScaleArgs args,
                                                             typename C::Aff* out) {
  using E = typename C::E;
  __shared__ E lds[(SCALE_GROUP - 1) * 3][SCALE_BLOCK];
  const uint32_t lane = threadIdx.x;
  // n < 2^31 and the grid covers n: nothing here overflows
  scale_lane<C>(pts, n, (uint64_t)blockIdx.x * SCALE_TILE + lane, SCALE_BLOCK, args,
                [&](int k) -> E& { return lds[k][lane]; }, out);
}

// ---- launcher (declared in g16_internal.hpp) ---------------------------------------------------------------------------
template <class C>
int32_t scale_uniform_device(g16_ctx* ctx, const void* d_pts, size_t n, const ScaleJob& job, void* d_out_aff) {
  if (!n) return G16_OK;
  ScaleArgs args;
  args.steps = job.d_steps, args.nsteps = job.nsteps, args.tail_dbls = job.tail_dbls;
  for (int q = 0; q < 8; ++q) args.k.v[q] = job.k_std[q];
  const uint32_t grid = (uint32_t)((n + SCALE_TILE - 1) / SCALE_TILE);
  KLAUNCH(ctx, sizeof(typename C::Aff) == sizeof(g1_aff) ? "scale_g1" : "scale_g2", scale_uniform<C>, grid, SCALE_BLOCK,
          0, (const typename C::Aff*)d_pts, (uint32_t)n, args, (typename C::Aff*)d_out_aff);
  HIPCHK(ctx, hipGetLastError());
  return G16_OK;
}

#endif   // __HIPCC__

}  // namespace g16
