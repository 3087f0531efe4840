// Kernels of the circuit setup (include/g16hip.h, "circuit setup"; host layer: circuit_setup.hip), templated over the
// curve C = G1 / G2 of ec.cuh, and their launchers.  Instantiated per curve in circuit_setup_g1.hip / _g2.hip.
//
//   cs_term       out[d] = k_e * P[src_e]: the one place a point meets a scalar -- the terms of a sparse product, the
//                 uniform delta^-1 scaling, and the load pass of the group NTT (d = the bit reversal of e)
//   cs_butterfly  one radix-2 stage of the group inverse NTT in place (circuit_setup_plan.hpp)
//   cs_segsum     per-wire sums of the sorted terms, lanes per wire by the bins of spmv_params.hpp
//   cs_to_affine  the working form (XYZZ) to canonical affine bytes
//   cs_diff       out[i] = P[i] - Q[i], affine (G1: the H points)
// A butterfly is one 254-bit scalar multiplication and two additions -- ~10^5 VALU instructions against 512 bytes (G1)
// moved: compute-bound by orders of magnitude, hence plain global memory and one lane per butterfly.  Every addition is
// the complete one of ec.cuh: powers of tau with tau in the domain make butterflies meet equal, opposite and infinite
// operands in every stage.
#pragma once
#include "circuit_setup_plan.hpp"
#include "g16_internal.hpp"
#include "scalar_mul.cuh"

namespace g16 {

// k * P for a canonical standard-form k: 0, 1 and r - 1 (most entries of a real circuit are +-1) without a ladder
template <class C>
__device__ typename C::Acc cs_scale(const typename C::Aff& p, const u256& k) {
  if (Fr::is_zero(k)) return C::acc_inf();
  u256 t = k;   // k == 1 or k == r - 1: every limb above the lowest agrees with that of 0 resp. r
  const bool hi_zero = !(k.v[1] | k.v[2] | k.v[3] | k.v[4] | k.v[5] | k.v[6] | k.v[7]);
  if (hi_zero && k.v[0] == 1u) return C::from_affine(p);
  t.v[0] += 1u;   // r is odd: no carry when k = r - 1
  if (k.v[0] != 0xffffffffu && Fr::eq(t, Fr::modulus())) return C::from_affine(C::neg(p));
  return scalar_mul<C>(p, k);
}

// entry e < count: point pts[src[e]] (src null: e), scalar val[vstride * ord[e]] (ord null: e; vstride 0: one scalar
// for all), Montgomery if `mont`; written to out[rev(e)] over log2rev bits (0: out[e])
template <class C>
__global__ void __launch_bounds__(CS_BLOCK) cs_term(const typename C::Aff* __restrict__ pts,
                                                    const uint32_t* __restrict__ src, const u256* __restrict__ val,
                                                    const uint32_t* __restrict__ ord, uint32_t vstride, uint32_t mont,
                                                    uint32_t log2rev, uint32_t count,
                                                    typename C::Acc* __restrict__ out) {
  const uint32_t e = blockIdx.x * CS_BLOCK + threadIdx.x;
  if (e >= count) return;
  u256 k = val[(size_t)vstride * (ord ? ord[e] : e)];
  if (mont) k = Fr::from_mont(k);
  out[log2rev ? pintt_rev(log2rev, e) : e] = cs_scale<C>(pts[src ? src[e] : e], k);
}

// stage s of the inverse NTT of v (2^log2n XYZZ points, in place); tw[k] = omega^-k in standard form, k < 2^(log2n-1)
template <class C>
__global__ void __launch_bounds__(CS_BLOCK) cs_butterfly(typename C::Acc* __restrict__ v, const u256* __restrict__ tw,
                                                         uint32_t log2n, uint32_t s) {
  const uint32_t t = blockIdx.x * CS_BLOCK + threadIdx.x;
  if (t >= pintt_butterflies(log2n)) return;
  const PinttPair pr = pintt_pair(log2n, s, t);
  typename C::Acc a = v[pr.lo], b = v[pr.hi];
  if (pr.tw) b = scalar_mul<C>(b, tw[pr.tw]);
  typename C::Acc sum = a;
  C::add(sum, b);
  C::add(a, C::neg(b));
  v[pr.lo] = sum;
  v[pr.hi] = a;
}

// wires[slot], slot < nw, sums its terms [off[w], off[w + 1]) with 2^glog lanes: each lane every 2^glog-th term, then a
// tree over the lanes through LDS; lane 0 writes the affine sum (no term: (0,0))
template <class C>
__global__ void __launch_bounds__(CS_BLOCK) cs_segsum(const typename C::Acc* __restrict__ terms,
                                                      const uint32_t* __restrict__ off,
                                                      const uint32_t* __restrict__ wires, uint32_t nw, uint32_t glog,
                                                      typename C::Aff* __restrict__ out) {
  __shared__ typename C::Acc sh[CS_BLOCK];
  const uint32_t t = blockIdx.x * CS_BLOCK + threadIdx.x;
  const uint32_t lanes = 1u << glog, slot = t >> glog, lane = t & (lanes - 1u);
  const bool live = slot < nw;
  const uint32_t w = live ? wires[slot] : 0u;
  typename C::Acc acc = C::acc_inf();
  if (live) {
    const uint32_t end = off[w + 1];
    for (uint32_t i = off[w] + lane; i < end; i += lanes) C::add(acc, terms[i]);
  }
  for (uint32_t h = lanes >> 1; h; h >>= 1) {   // glog is uniform over the grid: every lane takes every barrier
    sh[threadIdx.x] = acc;
    __syncthreads();
    if (lane < h) C::add(acc, sh[threadIdx.x + h]);
    __syncthreads();
  }
  if (live && lane == 0) out[w] = C::to_affine(acc);
}

template <class C>
__global__ void __launch_bounds__(CS_BLOCK) cs_to_affine(const typename C::Acc* __restrict__ in, uint32_t count,
                                                         typename C::Aff* __restrict__ out) {
  const uint32_t i = blockIdx.x * CS_BLOCK + threadIdx.x;
  if (i < count) out[i] = C::to_affine(in[i]);
}

template <class C>
__global__ void __launch_bounds__(CS_BLOCK) cs_diff(const typename C::Aff* __restrict__ p,
                                                    const typename C::Aff* __restrict__ q, uint32_t count,
                                                    typename C::Aff* __restrict__ out) {
  const uint32_t i = blockIdx.x * CS_BLOCK + threadIdx.x;
  if (i >= count) return;
  typename C::Acc acc = C::from_affine(p[i]);
  C::madd(acc, C::neg(q[i]));
  out[i] = C::to_affine(acc);
}

// ---- launchers (declared in g16_internal.hpp) ------------------------------------------------------------------------
template <class C>
constexpr const char* cs_name(const char* g1, const char* g2) {
  return sizeof(typename C::Aff) == sizeof(g1_aff) ? g1 : g2;
}

template <class C>
int32_t cs_term_device(g16_ctx* ctx, const void* d_pts, const uint32_t* d_src, const void* d_val, const uint32_t* d_ord,
                       uint32_t vstride, uint32_t mont, uint32_t log2rev, size_t count, void* d_out_acc) {
  if (!count) return G16_OK;
  KLAUNCH(ctx, cs_name<C>("setup_term_g1", "setup_term_g2"), cs_term<C>, cs_grid(count), CS_BLOCK, 0,
          (const typename C::Aff*)d_pts, d_src, (const u256*)d_val, d_ord, vstride, mont, log2rev, (uint32_t)count,
          (typename C::Acc*)d_out_acc);
  HIPCHK(ctx, hipGetLastError());
  return G16_OK;
}

template <class C>
int32_t cs_butterflies_device(g16_ctx* ctx, void* d_v, const void* d_tw, uint32_t log2n) {
  for (uint32_t s = 0; s < pintt_stages(log2n); ++s) {
    KLAUNCH(ctx, cs_name<C>("setup_butterfly_g1", "setup_butterfly_g2"), cs_butterfly<C>, pintt_stage_grid(log2n),
            CS_BLOCK, 0, (typename C::Acc*)d_v, (const u256*)d_tw, log2n, s);
    HIPCHK(ctx, hipGetLastError());
  }
  return G16_OK;
}

template <class C>
int32_t cs_segsum_device(g16_ctx* ctx, const void* d_terms, const uint32_t* d_off, const uint32_t* d_wires,
                         const CsSumPlan& plan, void* d_out_aff) {
  for (uint32_t b = 0; b < (uint32_t)NBINS; ++b) {
    if (!plan.count[b]) continue;
    KLAUNCH(ctx, cs_name<C>("setup_sum_g1", "setup_sum_g2"), cs_segsum<C>, plan.grid[b], CS_BLOCK, 0,
            (const typename C::Acc*)d_terms, d_off, d_wires + plan.first[b], plan.count[b], bin_glog(b),
            (typename C::Aff*)d_out_aff);
    HIPCHK(ctx, hipGetLastError());
  }
  return G16_OK;
}

template <class C>
int32_t cs_to_affine_device(g16_ctx* ctx, const void* d_acc, size_t count, void* d_out_aff) {
  if (!count) return G16_OK;
  KLAUNCH(ctx, cs_name<C>("setup_affine_g1", "setup_affine_g2"), cs_to_affine<C>, cs_grid(count), CS_BLOCK, 0,
          (const typename C::Acc*)d_acc, (uint32_t)count, (typename C::Aff*)d_out_aff);
  HIPCHK(ctx, hipGetLastError());
  return G16_OK;
}

template <class C>
int32_t cs_diff_device(g16_ctx* ctx, const void* d_p, const void* d_q, size_t count, void* d_out_aff) {
  if (!count) return G16_OK;
  KLAUNCH(ctx, "setup_diff", cs_diff<C>, cs_grid(count), CS_BLOCK, 0, (const typename C::Aff*)d_p,
          (const typename C::Aff*)d_q, (uint32_t)count, (typename C::Aff*)d_out_aff);
  HIPCHK(ctx, hipGetLastError());
  return G16_OK;
}

#define CS_INSTANTIATE(C)                                                                                              \
  template int32_t cs_term_device<C>(g16_ctx*, const void*, const uint32_t*, const void*, const uint32_t*, uint32_t, \
                                     uint32_t, uint32_t, size_t, void*);                                              \
  template int32_t cs_butterflies_device<C>(g16_ctx*, void*, const void*, uint32_t);                                  \
  template int32_t cs_segsum_device<C>(g16_ctx*, const void*, const uint32_t*, const uint32_t*, const CsSumPlan&,     \
                                       void*);                                                                         \
  template int32_t cs_to_affine_device<C>(g16_ctx*, const void*, size_t, void*);

}  // namespace g16
