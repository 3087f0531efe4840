// out[i] = k_i * P[i]: a scalar PER POINT (include/g16hip.h, "scaling an array of points"; host layer: scale.hip).  What
// scale.cuh does for one scalar, with everything that was wave-uniform there now the lane's own.  Instantiated per curve
// in scale_each_g1.hip / scale_each_g2.hip.
//
// G1.  The lane splits its scalar itself: k = k1 + k2 lambda, the Babai rounding of scale_split (scale_plan.hpp) in
// 32-bit limbs and modulo 2^160 (the halves lie inside (-2^128, 2^128), so five limbs hold them with their sign), without
// the identity check the host version carries: tests/test_phase1_cpu.py holds this very code to Python integers, and the
// bound with it.  The signs of the halves go into the table once -- A = s1 P, B = s2 phi P and A + B, which is
// +-(P + phi P) when the signs agree and +-(P - phi P) when they differ -- so a lane keeps three entries, not four, and a
// column of (|k1|, |k2|) selects by its two bits with no negation in the loop.  The table lives on the isomorphic curve
// E' exactly as in scale_ladder (scale.cuh): no division for P - phi P, dbl / madd of ec.cuh unchanged.  Plain bits, no
// sparse recoding: a column that is empty in all 64 lanes of a wave almost never happens, so the wave pays one doubling
// and one mixed addition per column whatever the digits -- what counts is the 128 columns against the 254 of the plain
// ladder.  A lane starts at its own top limb (doubling infinity returns at once), so short scalars pay for their own
// length, and for the wave's longest only by waiting.
// G2 has no endomorphism here: scalar_mul over the lane's own k.
// Affine output: scale_group of scale.cuh, four points per inversion, parked in LDS.
// The lane arithmetic is plain FF_HD code: tests/cpu_kernels/scale_each_shim.cpp runs it with g++ against the oracle.
#pragma once
#include "scale.cuh"

namespace g16 {

// limb q (32 bits) of a constant of scale_plan.hpp
constexpr uint32_t scale_limb(const U256& a, int q) { return (uint32_t)(a.v[q >> 1] >> (32 * (q & 1))); }

// w = a b truncated to NW limbs (schoolbook; a partial sum never exceeds 64 bits: (2^32 - 1)^2 + 2 (2^32 - 1))
template <int NA, int NB, int NW>
FF_HD void each_mul(const uint32_t (&a)[NA], const uint32_t (&b)[NB], uint32_t (&w)[NW]) {
#pragma unroll
  for (int i = 0; i < NW; ++i) w[i] = 0;
#pragma unroll
  for (int i = 0; i < NA; ++i) {
    uint64_t c = 0;
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      if (i + j < NW) {
        c += (uint64_t)a[i] * b[j] + w[i + j];
        w[i + j] = (uint32_t)c;
        c >>= 32;
      }
    }
    if (i + NB < NW) w[i + NB] = (uint32_t)c;
  }
}
// a -= b over five limbs, wrapping
FF_HD void each_sub(uint32_t (&a)[5], const uint32_t (&b)[5]) {
  uint32_t bw = 0;
#pragma unroll
  for (int i = 0; i < 5; ++i) {
    const uint64_t d = (uint64_t)a[i] - b[i] - bw;
    a[i] = (uint32_t)d;
    bw = (uint32_t)(d >> 63);
  }
}

struct EachSplit {
  uint32_t k1[4], k2[4];   // the magnitudes, little-endian
  bool neg1, neg2;
  bool ok;                 // both magnitudes below 2^128 (asserted on the CPU; the device never reads it)
};

// a two's-complement value of five limbs -> magnitude and sign; false if the magnitude needs the fifth limb
FF_HD bool each_abs(uint32_t (&v)[5], uint32_t (&mag)[4], bool& neg) {
  neg = (v[4] >> 31) != 0;
  uint32_t carry = neg ? 1u : 0u;
  const uint32_t flip = neg ? 0xffffffffu : 0u;
#pragma unroll
  for (int i = 0; i < 5; ++i) {
    const uint64_t s = (uint64_t)(v[i] ^ flip) + carry;
    v[i] = (uint32_t)s;
    carry = (uint32_t)(s >> 32);
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) mag[i] = v[i];
  return v[4] == 0;
}

// k canonical (< r), standard form
FF_HD EachSplit scale_each_split(const u256& k) {
  constexpr U256 NB1 = u256_neg(SCALE_B1);   // -b1 > 0
  const uint32_t g1[3] = {scale_limb(SCALE_G1, 0), scale_limb(SCALE_G1, 1), scale_limb(SCALE_G1, 2)};
  const uint32_t g2[5] = {scale_limb(SCALE_G2, 0), scale_limb(SCALE_G2, 1), scale_limb(SCALE_G2, 2),
                          scale_limb(SCALE_G2, 3), scale_limb(SCALE_G2, 4)};
  const uint32_t a1[2] = {scale_limb(SCALE_A1, 0), scale_limb(SCALE_A1, 1)};
  const uint32_t a2[4] = {scale_limb(SCALE_A2, 0), scale_limb(SCALE_A2, 1), scale_limb(SCALE_A2, 2),
                          scale_limb(SCALE_A2, 3)};
  const uint32_t nb1[4] = {scale_limb(NB1, 0), scale_limb(NB1, 1), scale_limb(NB1, 2), scale_limb(NB1, 3)};
  const uint32_t b2[2] = {scale_limb(SCALE_B2, 0), scale_limb(SCALE_B2, 1)};
  static_assert(!SCALE_G1.v[2] && !SCALE_G1.v[3] && !(SCALE_G1.v[1] >> 32) && !SCALE_G2.v[3] && !(SCALE_G2.v[2] >> 32) &&
                    !SCALE_A1.v[1] && !SCALE_A2.v[2] && !NB1.v[2] && !NB1.v[3] && !SCALE_B2.v[1],
                "a constant of the decomposition is longer than the limbs taken from it");
  uint32_t kk[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) kk[i] = k.v[i];
  // c1 = floor(g1 k / 2^256) < 2^64, c2 = floor(g2 k / 2^256) < 2^128 (g1 < 2^66, g2 < 2^130, k < 2^254)
  uint32_t w1[11], w2[13];
  each_mul(g1, kk, w1);
  each_mul(g2, kk, w2);
  const uint32_t c1[2] = {w1[8], w1[9]}, c2[4] = {w2[8], w2[9], w2[10], w2[11]};
  // k1 = k - c1 a1 - c2 a2, k2 = c1 (-b1) - c2 b2, modulo 2^160
  uint32_t v1[5] = {kk[0], kk[1], kk[2], kk[3], kk[4]}, v2[5], t[5];
  each_mul(c1, a1, t);
  each_sub(v1, t);
  each_mul(c2, a2, t);
  each_sub(v1, t);
  each_mul(c1, nb1, v2);
  each_mul(c2, b2, t);
  each_sub(v2, t);
  EachSplit s;
  const bool ok1 = each_abs(v1, s.k1, s.neg1), ok2 = each_abs(v2, s.k2, s.neg2);
  s.ok = ok1 && ok2;
  return s;
}

// k * p on G1; p on the curve or (0,0), k canonical, standard form
FF_HD g1_acc scale_each_ladder(const g1_aff& p, const u256& k) {
  if (G1::is_inf(p)) return G1::acc_inf();
  const EachSplit sp = scale_each_split(k);
  // the table on E' (scale.cuh): A = s1 P, B = s2 phi P, C = A + B
  const u256 t = Fp::mul(scale_beta_minus_one(), p.x);
  const u256 tt = Fp::sqr(t), ttt = Fp::mul(t, tt);
  u256 xa, xb, xc, ya, yb, yc;
  {
    const u256 y0 = Fp::mul(p.y, ttt);
    xa = Fp::mul(p.x, tt);
    xb = Fp::mul(scale_beta(), xa);
    ya = sp.neg1 ? Fp::neg(y0) : y0;
    yb = sp.neg2 ? Fp::neg(y0) : y0;
    if (sp.neg1 == sp.neg2) {   // s1 (P + phi P) = s1 (beta^2 x, -y)
      xc = Fp::mul(scale_beta_sqr(), xa);
      yc = Fp::neg(ya);
    } else {                    // s1 (P - phi P), by madd-2008-s from zz = zzz = 1 as in scale_ladder
      const u256 r = Fp::neg(Fp::dbl(p.y));
      xc = Fp::sub(Fp::sub(Fp::sqr(r), ttt), Fp::dbl(xa));
      yc = Fp::mulsub(r, Fp::sub(xa, xc), p.y, ttt);
      if (sp.neg1) yc = Fp::neg(yc);
    }
  }
  uint32_t a0 = sp.k1[0], a1 = sp.k1[1], a2 = sp.k1[2], a3 = sp.k1[3];
  uint32_t b0 = sp.k2[0], b1 = sp.k2[1], b2 = sp.k2[2], b3 = sp.k2[3];
  g1_acc acc = G1::acc_inf();
#pragma unroll 1
  for (int j = 3; j >= 0; --j) {
    const uint32_t la = a3, lb = b3;
    a3 = a2, a2 = a1, a1 = a0, a0 = la;   // rotate: no dynamic register index
    b3 = b2, b2 = b1, b1 = b0, b0 = lb;
    if (!(la | lb) && G1::is_inf(acc)) continue;
#pragma unroll 1
    for (int bit = 31; bit >= 0; --bit) {
      acc = G1::dbl(acc);
      const uint32_t col = ((la >> bit) & 1u) | (((lb >> bit) & 1u) << 1);
      if (!col) continue;
      g1_aff q;
      q.x = col == 1u ? xa : col == 2u ? xb : xc;
      q.y = col == 1u ? ya : col == 2u ? yb : yc;
      G1::madd(acc, q);
    }
  }
  // back to E: zz *= t^2, zzz *= t^3
  acc.zz = Fp::mul(acc.zz, tt);
  acc.zzz = Fp::mul(acc.zzz, ttt);
  return acc;
}
FF_HD g2_acc scale_each_ladder(const g2_aff& p, const u256& k) {
  return scalar_mul<G2>(p, k);
}

// scale_lane of scale.cuh with the scalar of point i at scalars[i] (Montgomery form if `mont`)
template <class C, class Park>
FF_HD void scale_each_lane(const typename C::Aff* pts, const u256* scalars, uint32_t mont, uint64_t n, uint64_t first,
                           uint64_t stride, Park park, typename C::Aff* out) {
  scale_group<C>(
      n, first, stride,
      [&](uint64_t i) {
        u256 k = scalars[i];
        if (mont) k = Fr::from_mont(k);
        return scale_each_ladder(pts[i], k);
      },
      park, out);
}

#if defined(__HIPCC__)
// The tile of scale_uniform.  No __restrict__ on the points: out may be pts.
template <class C>
__global__ void __launch_bounds__(SCALE_BLOCK) scale_each(const typename C::Aff* pts, const u256* __restrict__ scalars,
                                                          uint32_t mont, uint32_t n, typename C::Aff* out) {
  using E = typename C::E;
  __shared__ E lds[(SCALE_GROUP - 1) * 3][SCALE_BLOCK];
  const uint32_t lane = threadIdx.x;
  // n < 2^31 and the grid covers n: nothing here overflows
  scale_each_lane<C>(pts, scalars, mont, n, (uint64_t)blockIdx.x * SCALE_TILE + lane, SCALE_BLOCK,
                     [&](int k) -> E& { return lds[k][lane]; }, out);
}

// ---- launcher (declared in g16_internal.hpp) ---------------------------------------------------------------------------
template <class C>
int32_t scale_each_device(g16_ctx* ctx, const void* d_pts, size_t n, const void* d_scalars, uint32_t mont,
                          void* d_out_aff) {
  if (!n) return G16_OK;
  const uint32_t grid = (uint32_t)((n + SCALE_TILE - 1) / SCALE_TILE);
  KLAUNCH(ctx, sizeof(typename C::Aff) == sizeof(g1_aff) ? "scale_each_g1" : "scale_each_g2", scale_each<C>, grid,
          SCALE_BLOCK, 0, (const typename C::Aff*)d_pts, (const u256*)d_scalars, mont, (uint32_t)n,
          (typename C::Aff*)d_out_aff);
  HIPCHK(ctx, hipGetLastError());
  return G16_OK;
}
#endif   // __HIPCC__

}  // namespace g16
