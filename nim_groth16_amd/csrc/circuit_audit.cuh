// Kernels of the circuit audit (circuit_audit.hip): the glue between the kernels it drives -- buildABC's sparse
// products, the NTT, the one-shot MSM and the element passes of the key audit.
//   vec_first_mismatch   first index where two Fr vectors differ
//   widen_mask           16-byte multipliers -> 32-byte standard scalars, split into z|pub and z|priv
//   vec_add              elementwise sum of two Fr vectors
//   h_scatter            the coefficient-side vector of the H relation, both flavours
//   pairing_product<K>   prod_k e(+-P_k, Q_k) == 1, K <= 4
#pragma once
#include "pairing.cuh"

namespace g16 {

constexpr int CA_BLOCK = 256;

// *first (0xffffffff on entry) = the smallest i < n with a[i] != b[i].  Both vectors hold canonical residues in the same
// form, so equality of the field elements is equality of the limbs.
__global__ void __launch_bounds__(CA_BLOCK) vec_first_mismatch(const u256* __restrict__ a, const u256* __restrict__ b,
                                                               uint32_t n, uint32_t* __restrict__ first) {
  const uint32_t i = blockIdx.x * CA_BLOCK + threadIdx.x;
  if (i >= n) return;
  if (!Fr::eq(a[i], b[i])) atomicMin(first, i);
}

// z: nvars multipliers of 16 bytes.  whole[i] = z_i, pub[i] = z_i for i <= npubs else 0, priv[i] = z_i - pub[i], all as
// 32-byte standard-form scalars (a 128-bit value is below r).
__global__ void __launch_bounds__(CA_BLOCK) widen_mask(const uint4* __restrict__ z, uint32_t nvars, uint32_t npubs,
                                                       u256* __restrict__ whole, u256* __restrict__ pub,
                                                       u256* __restrict__ priv) {
  const uint32_t i = blockIdx.x * CA_BLOCK + threadIdx.x;
  if (i >= nvars) return;
  const uint4 w = z[i];
  u256 v, zero;
#pragma unroll
  for (int k = 0; k < 8; ++k) v.v[k] = zero.v[k] = 0;
  v.v[0] = w.x, v.v[1] = w.y, v.v[2] = w.z, v.v[3] = w.w;
  whole[i] = v;
  pub[i] = i <= npubs ? v : zero;
  priv[i] = i <= npubs ? zero : v;
}

// out[i] = a[i] + b[i] (Montgomery or standard alike)
__global__ void __launch_bounds__(CA_BLOCK) vec_add(const u256* __restrict__ a, const u256* __restrict__ b, uint32_t n,
                                                    u256* __restrict__ out) {
  const uint32_t i = blockIdx.x * CA_BLOCK + threadIdx.x;
  if (i >= n) return;
  out[i] = Fr::add(a[i], b[i]);
}

// The vector whose MSM against tauG1[0 .. 2n) must equal MSM(y, pointsH1) times delta; y: n multipliers of 16 bytes,
// out: 2n Fr in Montgomery form, ystd: the n multipliers as standard-form scalars (for the MSM against pointsH1).
//   snarkjs    pointsH1[i] = delta^-1 L_{2i+1}(tau) on the 2n-point domain: out = the VALUES v[2i+1] = y_i, v[2i] = 0,
//              which the caller turns into coefficients with one inverse NTT of 2n points
//   JensGroth  pointsH1[i] = delta^-1 (tau^n - 1) tau^i: out = the coefficients c[i] = -y_i, c[n+i] = y_i themselves
__global__ void __launch_bounds__(CA_BLOCK) h_scatter(const uint4* __restrict__ y, uint32_t n, uint32_t snarkjs,
                                                      u256* __restrict__ out, u256* __restrict__ ystd) {
  const uint32_t i = blockIdx.x * CA_BLOCK + threadIdx.x;
  if (i >= n) return;
  const uint4 w = y[i];
  u256 v;
#pragma unroll
  for (int k = 0; k < 8; ++k) v.v[k] = 0;
  v.v[0] = w.x, v.v[1] = w.y, v.v[2] = w.z, v.v[3] = w.w;
  ystd[i] = v;
  const u256 m = Fr::to_mont(v);
  if (snarkjs) {
    out[2 * (size_t)i] = Fr::zero();
    out[2 * (size_t)i + 1] = m;
  } else {
    out[i] = Fr::neg(m);
    out[(size_t)n + i] = m;
  }
}

// result[j] = ( prod_{k < K} e(s_k P[j][k], Q[j][k]) == 1 ), s_k = -1 where bit k of neg_mask is set.  (0,0) on either
// side of a pair contributes 1.  One workgroup per product: lanes 0 .. K-1 run one Miller loop each, lane 0 the product,
// the final exponentiation and the comparison.  It generalises audit_relation (audit.cuh), which is K = 2 with fixed
// generators.  Registers are per lane: K concurrent Miller loops in one wave take the registers of one, and the
// accumulators meet only in LDS (K x 384 bytes).
template <int K>
__global__ void __launch_bounds__(64) pairing_product(const g1_aff* __restrict__ P, const g2_aff* __restrict__ Q,
                                                      uint32_t neg_mask, int32_t* __restrict__ result) {
  static_assert(K >= 1 && K <= 4, "one lane per Miller loop, up to four");
  __shared__ fp12_t sh[K];
  const uint32_t j = blockIdx.x, lane = threadIdx.x;
  if (lane < K) {
    fp12_t f;
    g1_aff p = P[(size_t)j * K + lane];
    const g2_aff q = Q[(size_t)j * K + lane];
    if ((neg_mask >> lane) & 1) p = G1::neg(p);
    Pairing::miller(f, p, q);
    sh[lane] = f;
  }
  __syncthreads();
  if (lane) return;
  fp12_t acc = sh[0];
#pragma unroll 1
  for (int k = 1; k < K; ++k) {
    const fp12_t a = acc, m = sh[k];
    Pairing::mul(acc, a, m);
  }
  fp12_t f;
  Pairing::final_exp(f, acc);
  result[j] = Pairing::is_one(f) ? 1 : 0;
}

}  // namespace g16
