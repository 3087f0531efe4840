// k * P for ONE scalar k and many points P of G1 (scale.cuh: the delta^-1 rescaling of a phase-2 contribution), as DATA:
// the host decomposes k once and every lane walks the same schedule (no lane ever looks at a scalar bit), as
// subgroup_plan.hpp does for the constant r.  Plain C++17, no HIP: the CPU suite builds it with g++ and evaluates it.
//
// Decomposition.  BN254 has the endomorphism phi(x, y) = (beta x, y) = lambda (x, y), beta^3 = 1 in Fp, lambda^3 = 1
// in Fr.  k = k1 + k2 lambda (mod r) with |k1|, |k2| < 2^128, by Babai rounding against the short basis {(a1, b1),
// (a2, b2)} of {(x, y): x + y lambda = 0 mod r} that the extended Euclid on (r, lambda) yields (entries of 64 and 127
// bits).  The roundings are floor(g_i k / 2^256) with g_i = floor(2^256 n_i / r): below the exact quotient by less than
// 2 (the floor itself, and g_i's own truncation times k / 2^256 < 1/4), so (k1, k2) = x v1 + y v2 with x, y in [0, 2)
// and |k1| < 2 (|a1| + |a2|) = 0.87 * 2^128, |k2| likewise: the bound the plan asserts and the arrays are sized for.
// (Seen: up to 0.49 * 2^128, 127 bits; exact rounding would give 126.)
//
// Schedule.  The joint sparse form (Solinas) of (|k1|, |k2|): signed digits, most significant first, with at most one
// non-zero column in every two on average -- expected density 1/2, so nsteps ~ l/2 for halves of l bits (l <= 128:
// at most 129 columns, at most 129 steps; ~64 for a random k) beside ndbl <= 128 doublings.  The signs of k1 and k2 are
// folded into the digits.  A step means: double `dbls` times, then add sign * table[entry],
//   entry 0: P   1: phi P   2: P + phi P   3: P - phi P
// starting from infinity (so the first step has dbls = 0), and `tail_dbls` doublings follow the last addition.
#pragma once
#include <cstdint>

namespace g16 {

constexpr int SCALE_BLOCK = 64;   // lanes per workgroup of scale_uniform (scale.cuh)
constexpr int SCALE_GROUP = 4;    // points per lane = points that share one field inversion (Montgomery's trick)
constexpr int SCALE_TILE = SCALE_BLOCK * SCALE_GROUP;   // points per workgroup; point j of lane t: tile + j * BLOCK + t

enum ScaleEntry : uint8_t { SCALE_P = 0, SCALE_PHI = 1, SCALE_SUM = 2, SCALE_DIFF = 3 };

struct ScaleStep {
  uint8_t dbls;    // doublings before the addition
  uint8_t entry;   // ScaleEntry
  int8_t sign;     // +1 / -1
  uint8_t pad;
};
static_assert(sizeof(ScaleStep) == 4, "a step is one 32-bit word (the kernel loads it as such)");

struct ScalePlan {
  static constexpr int MAX_STEPS = 132;   // 129 columns at most
  int nsteps = 0;
  int ndbl = 0;        // doublings in all, the tail included (none before the first addition)
  int tail_dbls = 0;   // doublings after the last addition
  ScaleStep step[MAX_STEPS] = {};
};

// what a launch of scale_uniform needs beside the points: G1 walks the uploaded steps, G2 the bits of k
struct ScaleJob {
  const uint32_t* d_steps = nullptr;   // device: nsteps words (ScaleStep)
  uint32_t nsteps = 0, tail_dbls = 0;
  uint32_t k_std[8] = {};              // k in standard form, 32-bit limbs, little-endian
};

// ---- 256-bit integers as four 64-bit limbs, little-endian; arithmetic wraps mod 2^256 (two's complement) -------------
struct U256 {
  uint64_t v[4];
};
constexpr U256 SCALE_R = {{0x43e1f593f0000001ull, 0x2833e84879b97091ull, 0xb85045b68181585dull, 0x30644e72e131a029ull}};
// lambda = 0xb3c4d79d41a917585bfc41088d8daaa78b17ea66b99c90dd: the cube root of unity in Fr with lambda (x, y) =
// (beta x, y) for beta = SCALE_BETA, the cube root of unity in Fp below (standard form).  The other root of each
// side pairs with the other root of the other: tests/test_phase2_cpu.py holds lambda gen1 == (beta, 2).
constexpr U256 SCALE_LAMBDA = {{0x8b17ea66b99c90ddull, 0x5bfc41088d8daaa7ull, 0xb3c4d79d41a91758ull, 0}};
constexpr U256 SCALE_BETA = {{0x5763473177fffffeull, 0xd4f263f1acdb5c4full, 0x59e26bcea0d48bacull, 0}};
// the basis: a1 + b1 lambda = a2 + b2 lambda = 0 (mod r), a1 b2 - a2 b1 = r; b1 is negative (two's complement)
constexpr U256 SCALE_A1 = {{0x89d3256894d213e3ull, 0, 0, 0}};
constexpr U256 SCALE_B1 = {{0x7dee441482b0eed8ull, 0x90b27db71147a603ull, ~0ull, ~0ull}};
constexpr U256 SCALE_A2 = {{0x0be4e1541221250bull, 0x6f4d8248eeb859fdull, 0, 0}};
constexpr U256 SCALE_B2 = {{0x89d3256894d213e3ull, 0, 0, 0}};
// g1 = floor(2^256 b2 / r), g2 = floor(2^256 (-b1) / r)
constexpr U256 SCALE_G1 = {{0xd91d232ec7e0b3d7ull, 0x2ull, 0, 0}};
constexpr U256 SCALE_G2 = {{0x7a7bd9d4391eb18dull, 0x4ccef014a773d2cfull, 0x2ull, 0}};

constexpr bool u256_is_zero(const U256& a) { return !(a.v[0] | a.v[1] | a.v[2] | a.v[3]); }
constexpr bool u256_eq(const U256& a, const U256& b) {
  return a.v[0] == b.v[0] && a.v[1] == b.v[1] && a.v[2] == b.v[2] && a.v[3] == b.v[3];
}
constexpr bool u256_geq(const U256& a, const U256& b) {
  for (int i = 3; i >= 0; --i)
    if (a.v[i] != b.v[i]) return a.v[i] > b.v[i];
  return true;
}
constexpr U256 u256_add(const U256& a, const U256& b) {
  U256 r{};
  unsigned __int128 c = 0;
  for (int i = 0; i < 4; ++i) {
    c += (unsigned __int128)a.v[i] + b.v[i];
    r.v[i] = (uint64_t)c;
    c >>= 64;
  }
  return r;
}
constexpr U256 u256_neg(const U256& a) {
  const U256 n = {{~a.v[0], ~a.v[1], ~a.v[2], ~a.v[3]}};
  return u256_add(n, U256{{1, 0, 0, 0}});
}
constexpr U256 u256_sub(const U256& a, const U256& b) { return u256_add(a, u256_neg(b)); }
// the 512-bit product: lo = a b mod 2^256, hi = floor(a b / 2^256), both operands unsigned
constexpr void u256_mul_wide(const U256& a, const U256& b, U256& lo, U256& hi) {
  uint64_t w[8] = {};
  for (int i = 0; i < 4; ++i) {
    unsigned __int128 c = 0;
    for (int j = 0; j < 4; ++j) {
      c += (unsigned __int128)a.v[i] * b.v[j] + w[i + j];
      w[i + j] = (uint64_t)c;
      c >>= 64;
    }
    w[i + 4] = (uint64_t)c;
  }
  lo = U256{{w[0], w[1], w[2], w[3]}};
  hi = U256{{w[4], w[5], w[6], w[7]}};
}
// a b mod 2^256: right for two's-complement operands as well
constexpr U256 u256_mul_lo(const U256& a, const U256& b) {
  U256 lo{}, hi{};
  u256_mul_wide(a, b, lo, hi);
  return lo;
}
constexpr bool u256_negative(const U256& a) { return a.v[3] >> 63; }

// ---- arithmetic mod r on canonical values (the identity check and the checker; never on the device) ------------------
constexpr U256 fr_add(const U256& a, const U256& b) {
  const U256 s = u256_add(a, b);   // a, b < r < 2^254: no wrap
  return u256_geq(s, SCALE_R) ? u256_sub(s, SCALE_R) : s;
}
constexpr U256 fr_neg(const U256& a) { return u256_is_zero(a) ? a : u256_sub(SCALE_R, a); }
constexpr U256 fr_mul(const U256& a, const U256& b) {   // double-and-add over the bits of b
  U256 acc = {{0, 0, 0, 0}};
  for (int i = 255; i >= 0; --i) {
    acc = fr_add(acc, acc);
    if (b.v[i >> 6] >> (i & 63) & 1) acc = fr_add(acc, a);
  }
  return acc;
}

// the two halves: magnitudes below 2^128 and signs
struct ScaleSplit {
  unsigned __int128 k1, k2;
  bool neg1, neg2;
  bool ok;   // both magnitudes below 2^128 and k1 + k2 lambda == k (mod r)
};

constexpr ScaleSplit scale_split(const U256& k) {
  U256 lo{}, c1{}, c2{};
  u256_mul_wide(SCALE_G1, k, lo, c1);
  u256_mul_wide(SCALE_G2, k, lo, c2);
  // k1 = k - c1 a1 - c2 a2, k2 = -c1 b1 - c2 b2, wrapping: the true values are far inside (-2^255, 2^255)
  U256 k1 = u256_sub(u256_sub(k, u256_mul_lo(c1, SCALE_A1)), u256_mul_lo(c2, SCALE_A2));
  U256 k2 = u256_neg(u256_add(u256_mul_lo(c1, SCALE_B1), u256_mul_lo(c2, SCALE_B2)));
  ScaleSplit s{};
  s.neg1 = u256_negative(k1), s.neg2 = u256_negative(k2);
  if (s.neg1) k1 = u256_neg(k1);
  if (s.neg2) k2 = u256_neg(k2);
  s.ok = !(k1.v[2] | k1.v[3] | k2.v[2] | k2.v[3]);
  s.k1 = (unsigned __int128)k1.v[1] << 64 | k1.v[0];
  s.k2 = (unsigned __int128)k2.v[1] << 64 | k2.v[0];
  // the identity, mod r
  U256 m1 = {{k1.v[0], k1.v[1], 0, 0}}, m2 = {{k2.v[0], k2.v[1], 0, 0}};
  if (s.neg1) m1 = fr_neg(m1);
  if (s.neg2) m2 = fr_neg(m2);
  s.ok = s.ok && u256_eq(fr_add(m1, fr_mul(SCALE_LAMBDA, m2)), k);
  return s;
}

// the plan of a canonical k (< r); `ok` (optional) reports the assertions of the decomposition
constexpr ScalePlan make_scale_plan(const U256& k, bool* ok = nullptr) {
  const ScaleSplit sp = scale_split(k);
  if (ok) *ok = sp.ok;
  // joint sparse form of (k1, k2), least significant column first
  int8_t u1[130] = {}, u2[130] = {};
  int len = 0;
  unsigned __int128 a = sp.k1, b = sp.k2;
  int d1 = 0, d2 = 0;
  while (a || d1 || b || d2) {
    const int l1 = (int)(a & 7) + d1, l2 = (int)(b & 7) + d2;
    int x = 0, y = 0;
    if (l1 & 1) {
      x = 2 - (l1 & 3);
      if (((l1 & 7) == 3 || (l1 & 7) == 5) && (l2 & 3) == 2) x = -x;
    }
    if (l2 & 1) {
      y = 2 - (l2 & 3);
      if (((l2 & 7) == 3 || (l2 & 7) == 5) && (l1 & 3) == 2) y = -y;
    }
    if (2 * d1 == 1 + x) d1 = 1 - d1;
    if (2 * d2 == 1 + y) d2 = 1 - d2;
    a >>= 1, b >>= 1;
    u1[len] = (int8_t)(sp.neg1 ? -x : x), u2[len] = (int8_t)(sp.neg2 ? -y : y);
    ++len;
  }
  ScalePlan p;
  int dbls = 0;
  bool started = false;
  for (int i = len - 1; i >= 0; --i) {
    if (started) ++dbls, ++p.ndbl;
    if (!u1[i] && !u2[i]) continue;
    ScaleStep& st = p.step[p.nsteps++];
    st.dbls = (uint8_t)dbls;
    st.entry = !u2[i] ? SCALE_P : !u1[i] ? SCALE_PHI : u1[i] == u2[i] ? SCALE_SUM : SCALE_DIFF;
    st.sign = u1[i] ? u1[i] : u2[i];
    dbls = 0;
    started = true;
  }
  p.tail_dbls = dbls;
  return p;
}

// What a plan evaluates to, mod r: the coefficients of P and phi P are carried through the steps (start at zero, per
// step double `dbls` times and add sign * entry), then c1 + c2 lambda.  Uses none of the code that made the plan
// (checked again, digit by digit in Python integers, by tests/test_phase2_cpu.py).
constexpr U256 scale_plan_value(const ScalePlan& p) {
  U256 c1 = {{0, 0, 0, 0}}, c2 = {{0, 0, 0, 0}};
  const U256 one = {{1, 0, 0, 0}};
  auto dbl = [&]() { c1 = fr_add(c1, c1), c2 = fr_add(c2, c2); };
  for (int s = 0; s < p.nsteps; ++s) {
    for (int b = 0; b < p.step[s].dbls; ++b) dbl();
    const U256 d = p.step[s].sign > 0 ? one : fr_neg(one);
    const int e = p.step[s].entry;
    if (e != SCALE_PHI) c1 = fr_add(c1, d);
    if (e == SCALE_PHI || e == SCALE_SUM) c2 = fr_add(c2, d);
    if (e == SCALE_DIFF) c2 = fr_add(c2, fr_neg(d));
  }
  for (int b = 0; b < p.tail_dbls; ++b) dbl();
  return fr_add(c1, fr_mul(SCALE_LAMBDA, c2));
}
constexpr bool scale_plan_is(const ScalePlan& p, const U256& k) { return u256_eq(scale_plan_value(p), k); }

namespace scale_plan_selfcheck {
constexpr U256 K = {{0x0123456789abcdefull, 0xfedcba9876543210ull, 0x0f1e2d3c4b5a6978ull, 0x1a2b3c4d5e6f7081ull}};
static_assert(u256_eq(u256_sub(u256_mul_lo(SCALE_A1, SCALE_B2), u256_mul_lo(SCALE_A2, SCALE_B1)), SCALE_R),
              "the lattice basis does not have determinant r");
static_assert(u256_eq(fr_mul(fr_mul(SCALE_LAMBDA, SCALE_LAMBDA), SCALE_LAMBDA), U256{{1, 0, 0, 0}}), "lambda^3 != 1");
static_assert(scale_split(K).ok && scale_plan_is(make_scale_plan(K), K), "the plan of a sample scalar is not the scalar");
static_assert(make_scale_plan(U256{{0, 0, 0, 0}}).nsteps == 0, "k = 0 has steps");
}  // namespace scale_plan_selfcheck

}  // namespace g16
