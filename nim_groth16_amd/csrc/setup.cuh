// Scalar side of the fake circuit-specific trusted setup (reference groth16/fake_setup.nim:201-326), per element.
//
// Everything a setup needs besides `y ** gen` and the sparse column sums is a geometric sequence x_i = w0 * s^i taken
// through one of two maps, and one elementwise combination over the wires:
//   powers    out[i] = c * x_i                  JensGroth H scalars delta^-1 Z(tau) tau^i (fake_setup.nim:290-294):
//                                               w0 = 1, s = tau, c = delta^-1 (tau^n - 1)
//   lagrange  out[i] = c * x_i / (tau - x_i)    L_i(tau) on the 2^k domain (math/poly.nim:242-250): w0 = 1, s = omega_n,
//                                               c = (tau^n - 1) / n;  delta^-1 L_{2i+1}(tau) on the doubled domain
//                                               (fake_setup.nim:301-304): w0 = omega_2n, s = omega_2n^2,
//                                               c = delta^-1 (tau^2n - 1) / (2n): only the odd indices are formed
//   combine   beta A_j + alpha B_j + C_j, times gamma^-1 for the public wires j <= npubs (pointsIC) and delta^-1 for the
//             others (pointsC1) (fake_setup.nim:273-280)
// A thread owns a RUN of SETUP_RUN consecutive elements: it finds its first x with one short power, walks the run by
// multiplying with s, and in lagrange mode inverts the run's denominators with ONE Fr::inv (prefix products).  The loops
// over the run are fully unrolled with compile-time indices, so the prefix products live in registers.
//
// A zero denominator (tau = x_i) is the reference's assert "point should be outside the domain", not an arithmetic
// case: the run takes that factor as one, writes 0 for the element and reports its position; the kernel keeps the
// smallest one for the host.
//
// The same header compiles with g++ (tests/cpu_kernels/setup_shim.cpp), like ff.cuh and ec.cuh.
#pragma once
#include "ff.cuh"

namespace g16 {

constexpr int SETUP_RUN = 8;       // elements per thread
constexpr int SETUP_BLOCK = 256;   // threads per workgroup

// ceilingLog2(nconstraints + npubs + 1) (fake_setup.nim:203-206, misc.nim:43-47); the sum is taken in 64 bits
FF_HD uint32_t setup_log2_domain(uint32_t nconstraints, uint32_t npubs) {
  const uint64_t x = (uint64_t)nconstraints + npubs + 1;
  uint32_t k = 0;
  while ((uint64_t(1) << k) < x) ++k;
  return k;
}

// b^e, e < 2^32 (a run's first index: below 2^29)
FF_HD u256 setup_pow_u32(u256 b, uint32_t e) {
  u256 r = Fr::one();
  while (e) {
    if (e & 1) r = Fr::mul(r, b);
    e >>= 1;
    if (e) b = Fr::sqr(b);
  }
  return r;
}

// omega_(2^log2n) = gen28^(2^(28 - log2n)), Montgomery (math/domain.nim:26-33; the constant of ntt.cuh); log2n <= 28
FF_HD u256 setup_omega(uint32_t log2n) {
  u256 g;
  g.v[0] = 0x725b19f0u; g.v[1] = 0x9bd61b6eu; g.v[2] = 0x41112ed4u; g.v[3] = 0x402d111eu;
  g.v[4] = 0x8ef62abcu; g.v[5] = 0x00e0a7ebu; g.v[6] = 0xa58a7e85u; g.v[7] = 0x2a3c09f0u;
  u256 w = Fr::to_mont(g);
  for (uint32_t i = log2n; i < 28; ++i) w = Fr::sqr(w);
  return w;
}

// the backward half of a lagrange run, element K: inv = 1 / (d_0 ... d_K) on entry, 1 / (d_0 ... d_(K-1)) on exit.
// (Instantiated per element: the loop pragma gives up on a body of three products, and a loop that stays a loop
// indexes x and pre at run time, which puts them into scratch.)
template <int K, int M>
FF_HD void setup_lagrange_back_one(const u256 (&x)[M], const u256 (&pre)[M], u256& inv, const u256& c, const u256& tau,
                                   uint32_t zero_mask, uint32_t len, u256* out) {
  const bool live = (uint32_t)K < len;
  const bool z = (zero_mask >> K) & 1u;
  u256 dinv = inv;   // 1 / d_K
  if constexpr (K > 0) {
    u256 d = Fr::sub(tau, x[K]);
    if (z || !live) d = Fr::one();
    dinv = Fr::mul(inv, pre[K - 1]);
    inv = Fr::mul(inv, d);
  }
  if (live) out[K] = z ? Fr::zero() : Fr::mul(Fr::mul(c, x[K]), dinv);
}
template <int M, int... I>
FF_HD void setup_lagrange_back(const u256 (&x)[M], const u256 (&pre)[M], u256& inv, const u256& c, const u256& tau,
                               uint32_t zero_mask, uint32_t len, u256* out, std::integer_sequence<int, I...>) {
  (setup_lagrange_back_one<M - 1 - I, M>(x, pre, inv, c, tau, zero_mask, len, out), ...);
}

// One run: elements k < len <= M of the sequence x_k = x0 * s^k, written to out[k] (nothing at or beyond out[len]).
// Returns the smallest k whose denominator is zero (lagrange mode), or M if there is none.
template <int M, bool LAGRANGE>
FF_HD uint32_t setup_geom_run(const u256& x0, const u256& s, const u256& c, const u256& tau, uint32_t len, u256* out) {
  if constexpr (!LAGRANGE) {
    u256 x = x0;
#pragma unroll
    for (int k = 0; k < M; ++k) {
      if ((uint32_t)k < len) out[k] = Fr::mul(c, x);
      if (k + 1 < M) x = Fr::mul(x, s);
    }
    return (uint32_t)M;
  } else {
    u256 x[M], pre[M];   // x_k and the product of the denominators 0..k, zero or absent ones taken as one
    uint32_t zero_mask = 0;
#pragma unroll
    for (int k = 0; k < M; ++k) {
      x[k] = k == 0 ? x0 : Fr::mul(x[k - 1], s);
      u256 d = Fr::sub(tau, x[k]);
      const bool live = (uint32_t)k < len;
      const bool z = live && Fr::is_zero(d);
      if (z) zero_mask |= 1u << k;
      if (z || !live) d = Fr::one();
      pre[k] = k == 0 ? d : Fr::mul(pre[k - 1], d);
    }
    u256 inv = Fr::inv(pre[M - 1]);   // of a product of non-zero factors
    setup_lagrange_back(x, pre, inv, c, tau, zero_mask, len, out, std::make_integer_sequence<int, M>{});
    uint32_t first = (uint32_t)M;
#pragma unroll
    for (int k = M - 1; k >= 0; --k)
      if ((zero_mask >> k) & 1u) first = (uint32_t)k;
    return first;
  }
}

// wire j of the combination (fake_setup.nim:273-280): (beta a + alpha b + c) / gamma for j <= npubs, / delta beyond
FF_HD u256 setup_combine(const u256& a, const u256& b, const u256& c, const u256& alpha, const u256& beta,
                         const u256& gamma_inv, const u256& delta_inv, uint32_t j, uint32_t npubs) {
  const u256 comb = Fr::add(Fr::mul2(beta, a, alpha, b), c);
  return Fr::mul(j <= npubs ? gamma_inv : delta_inv, comb);
}

}  // namespace g16
