// Verifier side of the C ABI: batched Groth16 verification and the raw pairing (verifier.nim:31-52,
// curves.nim:218-221).  One lane per pairing / per proof; see pairing.cuh.  Not a hot path of the prover --
// it exists so that a user of the reference's verifyProof finds it here, running on the same device.
#include "g16_internal.hpp"
#include "pairing.cuh"
#include "scalar_mul.cuh"   // scalar_mul: k * P over a canonical 254-bit scalar

using namespace g16;

struct g16_vkey {
  int device = 0;
  uint32_t npubs = 0;
  g2_aff gamma2, delta2;
  DevMem<> d_ic;   // (npubs + 1) G1 points
  DevMem<> d_ab;   // Miller value of (alpha1, beta2): 384 B
};

namespace {

constexpr int PBLOCK = 64;

__device__ bool on_curve_g1(const g1_aff& p) {
  if (G1::is_inf(p)) return true;
  u256 three = Fp::add(Fp::dbl(Fp::one()), Fp::one());
  return Fp::eq(Fp::sqr(p.y), Fp::add(Fp::mul(Fp::sqr(p.x), p.x), three));
}
__device__ bool on_curve_g2(const g2_aff& p, const fp2_t& b) {
  if (G2::is_inf(p)) return true;
  return Fp2::eq(Fp2::sqr(p.y), Fp2::add(Fp2::mul(Fp2::sqr(p.x), p.x), b));
}

// partial[j * (npubs+1) + i] = publicIO[j][i] * IC[i]
__global__ void __launch_bounds__(PBLOCK) verify_pub_terms(const u256* __restrict__ pub, uint32_t mont,
                                                           const g1_aff* __restrict__ ic, uint32_t nio,
                                                           uint32_t total, g1_acc* __restrict__ partial,
                                                           int32_t* __restrict__ status) {
  uint32_t t = blockIdx.x * PBLOCK + threadIdx.x;
  if (t >= total) return;
  u256 s = pub[t];
  if (!Fr::is_canonical(s)) atomicMin(&status[t / nio], -6);   // one public input, one accepted encoding
  if (mont) s = Fr::from_mont(s);
  partial[t] = scalar_mul<G1>(ic[t % nio], s);
}

// three Miller loops per proof: (-A, B), (C, delta), (vk_x, gamma); status < 0 on malformed input
__global__ void __launch_bounds__(PBLOCK) verify_miller(const g16_proof* __restrict__ proofs, uint32_t count,
                                                        const g1_acc* __restrict__ partial, uint32_t nio,
                                                        g2_aff gamma2, g2_aff delta2, fp2_t twist_b,
                                                        uint32_t check_subgroup, fp12_t* __restrict__ mil,
                                                        int32_t* __restrict__ status) {
  uint32_t t = blockIdx.x * PBLOCK + threadIdx.x;
  if (t >= 3 * count) return;
  const uint32_t j = t / 3, which = t % 3;
  const g16_proof& pr = proofs[j];
  g1_aff P;
  g2_aff Q;
  if (which == 0) {
    P = *reinterpret_cast<const g1_aff*>(pr.pi_a);
    Q = *reinterpret_cast<const g2_aff*>(pr.pi_b);
    // every coordinate must be the canonical residue (< p): the field arithmetic below would silently reduce a
    // larger limb pattern, so without this one proof would have several accepted byte encodings
    if (!Fp::is_canonical(P.x) || !Fp::is_canonical(P.y) || !Fp::is_canonical(Q.x.c0) || !Fp::is_canonical(Q.x.c1) ||
        !Fp::is_canonical(Q.y.c0) || !Fp::is_canonical(Q.y.c1))
      atomicMin(&status[j], -5);
    if (!on_curve_g1(P)) atomicMin(&status[j], -1);
    if (!on_curve_g2(Q, twist_b)) {
      atomicMin(&status[j], -2);
    } else if (check_subgroup) {   // [r]Q == infinity (the reference only asserts the curve equation)
      u256 r{{FrParams::P0, FrParams::P1, FrParams::P2, FrParams::P3, FrParams::P4, FrParams::P5, FrParams::P6,
              FrParams::P7}};
      if (!G2::is_inf(scalar_mul<G2>(Q, r))) atomicMin(&status[j], -4);
    }
    P = G1::neg(P);
  } else if (which == 1) {
    P = *reinterpret_cast<const g1_aff*>(pr.pi_c);
    Q = delta2;
    if (!Fp::is_canonical(P.x) || !Fp::is_canonical(P.y)) atomicMin(&status[j], -5);
    if (!on_curve_g1(P)) atomicMin(&status[j], -3);
  } else {
    g1_acc acc = G1::acc_inf();
    for (uint32_t i = 0; i < nio; ++i) G1::add(acc, partial[(size_t)j * nio + i]);
    P = G1::to_affine(acc);
    Q = gamma2;
  }
  Pairing::miller(mil[t], P, Q);
}

// status[j] = (m0 m1 m2 ab)^((p^12-1)/r) == 1, unless already negative
__global__ void __launch_bounds__(PBLOCK) verify_final(const fp12_t* __restrict__ mil, const fp12_t* __restrict__ ab,
                                                       uint32_t count, int32_t* __restrict__ status) {
  uint32_t j = blockIdx.x * PBLOCK + threadIdx.x;
  if (j >= count || status[j] < 0) return;
  fp12_t f, t;
  Pairing::mul(t, mil[3 * j], mil[3 * j + 1]);
  Pairing::mul(f, t, mil[3 * j + 2]);
  Pairing::mul(t, f, *ab);
  Pairing::final_exp(f, t);
  status[j] = Pairing::is_one(f) ? 1 : 0;
}

// ---- g16_verify_batch: one pairing-product check per batch ----------------------------------------------------------
//   prod_j e(-z_j A_j, B_j) * e(sum_j z_j C_j, delta2) * e(sum_i s_i IC_i, gamma2) * e(Z alpha1, beta2) == 1,
//   s_i = sum_j z_j pub_{j,i}, Z = sum_j z_j (mod r).
// One lane per item as above.  Every kernel here is one round of waves at the batch sizes in use, so a call costs the
// sum of its kernels' single-lane latencies: lanes with different jobs therefore sit in different WORKGROUPS of one
// launch (the five kinds of scalar multiplication in batch_scale, the Miller loops beside the order-r checks in
// batch_miller), never behind each other in one lane.

// k * P for a 128-bit multiplier (four limbs, little-endian)
template <class C>
__device__ typename C::Acc scalar_mul128(const typename C::Aff& p, uint4 k) {
  typename C::Acc acc = C::acc_inf();
#pragma unroll 1
  for (int j = 3; j >= 0; --j) {
    uint32_t limb = k.w;   // rotate: static register indices
    k.w = k.z;
    k.z = k.y;
    k.y = k.x;
    k.x = limb;
#pragma unroll 1
    for (int b = 31; b >= 0; --b) {
      acc = C::dbl(acc);
      if ((limb >> b) & 1) C::madd(acc, p);
    }
  }
  return acc;
}

// Block i < nio: s[i] = sum_j z_j pub[j][i]; block nio: s[nio] = sum_j z_j.  Canonical, standard form.
// A public input >= r gives its proof the code -6 and adds nothing.
__global__ void __launch_bounds__(PBLOCK) batch_fold_pub(const u256* __restrict__ pub, uint32_t mont,
                                                         const uint4* __restrict__ z, uint32_t nio, uint32_t count,
                                                         u256* __restrict__ s, int32_t* __restrict__ status) {
  __shared__ u256 sh[PBLOCK];
  const uint32_t i = blockIdx.x, lane = threadIdx.x;
  u256 acc = Fr::zero();
  for (uint32_t j = lane; j < count; j += PBLOCK) {
    const uint4 zj = z[j];
    u256 zr = Fr::zero();   // z_j < 2^128 < r as plain limbs
    zr.v[0] = zj.x;
    zr.v[1] = zj.y;
    zr.v[2] = zj.z;
    zr.v[3] = zj.w;
    if (i == nio) {
      acc = Fr::add(acc, zr);
      continue;
    }
    const u256 p = pub[(size_t)j * nio + i];
    if (!Fr::is_canonical(p)) {
      atomicMin(&status[j], -6);
      continue;
    }
    acc = Fr::add(acc, Fr::mul(zr, p));   // z * (p R) / R = z p for Montgomery p; z p / R for standard p
  }
  sh[lane] = acc;
  __syncthreads();
  for (uint32_t w = PBLOCK / 2; w; w >>= 1) {
    if (lane < w) sh[lane] = Fr::add(sh[lane], sh[lane + w]);
    __syncthreads();
  }
  if (lane == 0) s[i] = (i == nio || mont) ? sh[0] : Fr::to_mont(sh[0]);
}

// The scalar multiplications of a batch, one kind per range of workgroups (nb = workgroups per `count` lanes):
//   [0, nb)        lane j: checks of pi_a and pi_b (not the order of pi_b), nega[j] = z_j (-A_j), affine
//   [nb, 2 nb)     lane j: checks of pi_c, zc[j] = z_j C_j
//   [2 nb, last)   lane i: icp[i] = s_i IC_i
//   last           one lane: fixed_p[2] = Z alpha1, affine
// Codes and their order as in verify_miller.  A point that fails a check is replaced by infinity: nothing that is
// off its curve reaches an addition or a Miller loop.
__global__ void __launch_bounds__(PBLOCK) batch_scale(const g16_proof* __restrict__ proofs,
                                                      const uint4* __restrict__ z, uint32_t count,
                                                      const u256* __restrict__ s, const g1_aff* __restrict__ ic,
                                                      uint32_t nio, const g1_aff* __restrict__ alpha1, fp2_t twist_b,
                                                      g1_aff* __restrict__ nega, g1_acc* __restrict__ zc,
                                                      g1_acc* __restrict__ icp, g1_aff* __restrict__ fixed_p,
                                                      int32_t* __restrict__ status) {
  const uint32_t nb = (count + PBLOCK - 1) / PBLOCK, lane = threadIdx.x;
  uint32_t b = blockIdx.x;
  if (b < 2 * nb) {
    const bool is_c = b >= nb;
    const uint32_t j = (is_c ? b - nb : b) * PBLOCK + lane;
    if (j >= count) return;
    const g16_proof& pr = proofs[j];
    g1_aff P = *reinterpret_cast<const g1_aff*>(is_c ? pr.pi_c : pr.pi_a);
    bool ok = true;
    if (!Fp::is_canonical(P.x) || !Fp::is_canonical(P.y)) {
      atomicMin(&status[j], -5);
      ok = false;
    }
    if (!on_curve_g1(P)) {
      atomicMin(&status[j], is_c ? -3 : -1);
      ok = false;
    }
    if (!is_c) {
      const g2_aff Q = *reinterpret_cast<const g2_aff*>(pr.pi_b);
      if (!Fp::is_canonical(Q.x.c0) || !Fp::is_canonical(Q.x.c1) || !Fp::is_canonical(Q.y.c0) ||
          !Fp::is_canonical(Q.y.c1)) {
        atomicMin(&status[j], -5);
        ok = false;
      }
      if (!on_curve_g2(Q, twist_b)) {
        atomicMin(&status[j], -2);
        ok = false;
      }
    }
    g1_acc acc = G1::acc_inf();
    if (ok) acc = scalar_mul128<G1>(is_c ? P : G1::neg(P), z[j]);
    if (is_c) zc[j] = acc;
    else nega[j] = G1::to_affine(acc);
    return;
  }
  b -= 2 * nb;
  const uint32_t i = b * PBLOCK + lane;
  if (i < nio) icp[i] = scalar_mul<G1>(ic[i], s[i]);
  else if (i == ((nio + PBLOCK - 1) / PBLOCK) * PBLOCK) fixed_p[2] = G1::to_affine(scalar_mul<G1>(*alpha1, s[nio]));
}

// Sums of G1 accumulators: blockIdx.y picks the sum, every lane first adds up the elements one grid apart, then a
// tree through LDS.  With `fin` the workgroup's sum goes out as an affine point, else as a partial sum.
struct G1Sum {
  const g1_acc* in;
  uint32_t n;
  const int32_t* status;   // NULL, or: element j counts only while status[j] >= 0
  g1_acc* part;
  g1_aff* fin;
};
__global__ void __launch_bounds__(PBLOCK) batch_g1_sum(G1Sum s0, G1Sum s1) {
  __shared__ g1_acc sh[PBLOCK];
  const G1Sum& s = blockIdx.y ? s1 : s0;
  const uint32_t lane = threadIdx.x;
  g1_acc acc = G1::acc_inf();
  for (size_t t = (size_t)blockIdx.x * PBLOCK + lane; t < s.n; t += (size_t)gridDim.x * PBLOCK)
    if (!s.status || s.status[t] >= 0) G1::add(acc, s.in[t]);
  sh[lane] = acc;
  __syncthreads();
  for (uint32_t w = PBLOCK / 2; w; w >>= 1) {
    if (lane < w) {
      const g1_acc other = sh[lane + w];
      G1::add(acc, other);
      sh[lane] = acc;
    }
    __syncthreads();
  }
  if (lane) return;
  if (s.fin) *s.fin = G1::to_affine(acc);
  else s.part[blockIdx.x] = acc;
}

// Workgroups [0, nbm): lane t < count: mil[t] = miller(z_t (-A_t), B_t); the three lanes after them: (sum z C, delta2), (sum s IC, gamma2), (Z alpha1, beta2).
// Workgroups from nbm on: lane j: [r] B_j == infinity, else -4 (B_j on its curve: batch_scale gave -2 otherwise).
__global__ void __launch_bounds__(PBLOCK) batch_miller(const g16_proof* __restrict__ proofs, uint32_t count,
                                                       const g1_aff* __restrict__ nega,
                                                       const g1_aff* __restrict__ fixed_p, g2_aff delta2, g2_aff gamma2,
                                                       const g2_aff* __restrict__ beta2, fp2_t twist_b,
                                                       fp12_t* __restrict__ mil, int32_t* __restrict__ status) {
  const uint32_t nbm = (count + 3 + PBLOCK - 1) / PBLOCK;
  if (blockIdx.x >= nbm) {
    const uint32_t j = (blockIdx.x - nbm) * PBLOCK + threadIdx.x;
    if (j >= count) return;
    const g2_aff Q = *reinterpret_cast<const g2_aff*>(proofs[j].pi_b);
    if (!on_curve_g2(Q, twist_b)) return;
    u256 r{{FrParams::P0, FrParams::P1, FrParams::P2, FrParams::P3, FrParams::P4, FrParams::P5, FrParams::P6,
            FrParams::P7}};
    if (!G2::is_inf(scalar_mul<G2>(Q, r))) atomicMin(&status[j], -4);
    return;
  }
  const uint32_t t = blockIdx.x * PBLOCK + threadIdx.x;
  if (t >= count + 3) return;
  g1_aff P;
  g2_aff Q;
  if (t < count) {
    P = nega[t];   // infinity if pi_a or pi_b failed a check of batch_scale
    Q = *reinterpret_cast<const g2_aff*>(proofs[t].pi_b);
  } else {
    P = fixed_p[t - count];
    Q = t == count ? delta2 : t == count + 1 ? gamma2 : *beta2;
  }
  Pairing::miller(mil[t], P, Q);
}

// Product of Fp12 values, shaped like batch_g1_sum: out[blockIdx.x] = product of this workgroup's elements; with
// `status`, element t < count is left out while status[t] < 0
__global__ void __launch_bounds__(PBLOCK) batch_gt_product(const fp12_t* __restrict__ in, uint32_t n,
                                                           const int32_t* __restrict__ status, uint32_t count,
                                                           fp12_t* __restrict__ out) {
  __shared__ fp12_t sh[PBLOCK];
  const uint32_t lane = threadIdx.x;
  fp12_t acc = Pairing::one(), a;
  for (size_t t = (size_t)blockIdx.x * PBLOCK + lane; t < n; t += (size_t)gridDim.x * PBLOCK) {
    if (status && t < count && status[t] < 0) continue;
    a = acc;
    const fp12_t b = in[t];
    Pairing::mul(acc, a, b);
  }
  sh[lane] = acc;
  __syncthreads();
  for (uint32_t w = PBLOCK / 2; w; w >>= 1) {
    if (lane < w) {
      a = acc;
      const fp12_t b = sh[lane + w];
      Pairing::mul(acc, a, b);
      sh[lane] = acc;
    }
    __syncthreads();
  }
  if (lane == 0) out[blockIdx.x] = acc;
}

// *result = no proof has a negative code and f^((p^12-1)/r) == 1.  One workgroup.
__global__ void __launch_bounds__(PBLOCK) batch_final(const fp12_t* __restrict__ f, const int32_t* __restrict__ status,
                                                      uint32_t count, int32_t* __restrict__ result) {
  int bad = 0;
  for (uint32_t j = threadIdx.x; j < count; j += PBLOCK) bad |= status[j] < 0;
  bad = __syncthreads_or(bad);
  if (threadIdx.x) return;
  int32_t ok = 0;
  if (!bad) {
    fp12_t g;
    Pairing::final_exp(g, *f);
    ok = Pairing::is_one(g) ? 1 : 0;
  }
  *result = ok;
}

__global__ void __launch_bounds__(PBLOCK) pairing_kernel(const g1_aff* __restrict__ p, const g2_aff* __restrict__ q,
                                                         uint32_t n, int do_final, fp12_t* __restrict__ out) {
  uint32_t t = blockIdx.x * PBLOCK + threadIdx.x;
  if (t >= n) return;
  fp12_t f;
  Pairing::miller(f, p[t], q[t]);
  if (do_final) {
    fp12_t g = f;
    Pairing::final_exp(f, g);
  }
  out[t] = f;
}

u256 std_fp(uint32_t a7, uint32_t a6, uint32_t a5, uint32_t a4, uint32_t a3, uint32_t a2, uint32_t a1, uint32_t a0) {
  u256 v;
  v.v[0] = a0; v.v[1] = a1; v.v[2] = a2; v.v[3] = a3; v.v[4] = a4; v.v[5] = a5; v.v[6] = a6; v.v[7] = a7;
  return Fp::to_mont(v);   // standard form -> Montgomery
}
fp2_t twist_b() {   // twistCoeffB = 3/(9+u) (curves.nim:75-77)
  fp2_t b;
  b.c0 = std_fp(0x2b149d40u, 0xceb8aaaeu, 0x81be1899u, 0x1be06ac3u, 0xb5b4c5e5u, 0x59dbefa3u, 0x3267e6dcu, 0x24a138e5u);
  b.c1 = std_fp(0x009713b0u, 0x3af0fed4u, 0xcd2cafadu, 0xeed8fdf4u, 0xa74fa084u, 0xe52d1852u, 0xe4a2bd06u, 0x85c315d2u);
  return b;
}

}  // namespace

extern "C" int32_t g16_pairing(g16_ctx* ctx, const void* g1_points, const void* g2_points, size_t n, void* out_gt) {
  if (!ctx) return G16_EINVAL;
  if ((n && (!g1_points || !g2_points || !out_gt)) || n >= (size_t(1) << 24)) {
    ctx->err = "g16_pairing: bad arguments";
    return G16_EINVAL;
  }
  if (!n) return G16_OK;
  CTX_ENTER(ctx);
  int32_t rc;
  const size_t o_q = n * 64, o_out = o_q + n * 128;
  if ((rc = ensure(ctx, ctx->stage_p, o_out + n * sizeof(fp12_t)))) return rc;
  char* ws = (char*)ctx->stage_p.p();
  HIPCHK(ctx, hipMemcpyAsync(ws, g1_points, n * 64, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(ws + o_q, g2_points, n * 128, hipMemcpyHostToDevice, ctx->stream));
  KLAUNCH(ctx, "pairing", pairing_kernel, (uint32_t)((n + PBLOCK - 1) / PBLOCK), PBLOCK, 0, (const g1_aff*)ws,
          (const g2_aff*)(ws + o_q), (uint32_t)n, 1, (fp12_t*)(ws + o_out));
  HIPCHK(ctx, hipGetLastError());
  HIPCHK(ctx, hipMemcpyAsync(out_gt, ws + o_out, n * sizeof(fp12_t), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return G16_OK;
}

extern "C" int32_t g16_vkey_create(g16_ctx* ctx, const g16_vkey_desc* d, g16_vkey** out) {
  if (!ctx) return G16_EINVAL;
  if (!d || !out || !d->alpha1 || !d->beta2 || !d->gamma2 || !d->delta2 || !d->pointsIC || d->npubs >= (1u << 20)) {
    ctx->err = "g16_vkey_create: bad descriptor";
    return G16_EINVAL;
  }
  CTX_ENTER(ctx);
  Building<g16_vkey, g16_vkey_destroy> k(new (std::nothrow) g16_vkey());
  if (!k) return G16_ENOMEM;
  k->device = ctx->device;
  k->npubs = d->npubs;
  memcpy(&k->gamma2, d->gamma2, 128);
  memcpy(&k->delta2, d->delta2, 128);
  const size_t nio = (size_t)d->npubs + 1;
  HIPCHK(ctx, dev_alloc(k->d_ic, nio * 64));
  HIPCHK(ctx, dev_alloc(k->d_ab, sizeof(fp12_t) + 64 + 128));
  char* ab = (char*)k->d_ab.get();
  HIPCHK(ctx, hipMemcpyAsync(k->d_ic.get(), d->pointsIC, nio * 64, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(ab + sizeof(fp12_t), d->alpha1, 64, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(ab + sizeof(fp12_t) + 64, d->beta2, 128, hipMemcpyHostToDevice, ctx->stream));
  // vkey.spec.alphaBeta (zkey_types.nim:62-73) is kept as its Miller value; the final exponentiation is shared
  hipLaunchKernelGGL(pairing_kernel, dim3(1), dim3(PBLOCK), 0, ctx->stream, (const g1_aff*)(ab + sizeof(fp12_t)),
                     (const g2_aff*)(ab + sizeof(fp12_t) + 64), 1u, 0, (fp12_t*)ab);
  HIPCHK(ctx, hipGetLastError());
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  *out = k.release();
  return G16_OK;
}

extern "C" void g16_vkey_destroy(g16_vkey* k) {
  if (!k) return;
  (void)hipSetDevice(k->device);   // device-bound like g16_pkey: valid before and after any context
  (void)hipDeviceSynchronize();
  delete k;
}

extern "C" int32_t g16_verify(g16_ctx* ctx, const g16_vkey* key, const g16_proof* proofs, const void* public_io,
                              uint32_t flags, size_t count, int32_t* status) {
  if (!ctx) return G16_EINVAL;
  if (!key || key->device != ctx->device || (count && (!proofs || !public_io || !status)) || count >= (size_t(1) << 22)) {
    ctx->err = "g16_verify: bad arguments";
    return G16_EINVAL;
  }
  if (!count) return G16_OK;
  CTX_ENTER(ctx);
  const size_t nio = (size_t)key->npubs + 1, total = count * nio;
  size_t o = 0;
  auto take = [&](size_t bytes) {
    size_t r = o;
    o += (bytes + 255) & ~size_t(255);
    return r;
  };
  const size_t o_pr = take(count * sizeof(g16_proof)), o_pub = take(total * 32), o_part = take(total * sizeof(g1_acc)),
               o_mil = take(3 * count * sizeof(fp12_t)), o_st = take(count * 4);
  int32_t rc;
  if ((rc = ensure(ctx, ctx->stage_p, o))) return rc;
  char* ws = (char*)ctx->stage_p.p();
  HIPCHK(ctx, hipMemcpyAsync(ws + o_pr, proofs, count * sizeof(g16_proof), hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(ws + o_pub, public_io, total * 32, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipMemsetAsync(ws + o_st, 0, count * 4, ctx->stream));
  KLAUNCH(ctx, "verify_pub_terms", verify_pub_terms, (uint32_t)((total + PBLOCK - 1) / PBLOCK), PBLOCK, 0,
          (const u256*)(ws + o_pub), (flags & G16_SCALARS_MONT) ? 1u : 0u, (const g1_aff*)key->d_ic.get(), (uint32_t)nio,
          (uint32_t)total, (g1_acc*)(ws + o_part), (int32_t*)(ws + o_st));
  KLAUNCH(ctx, "verify_miller", verify_miller, (uint32_t)((3 * count + PBLOCK - 1) / PBLOCK), PBLOCK, 0,
          (const g16_proof*)(ws + o_pr), (uint32_t)count, (const g1_acc*)(ws + o_part), (uint32_t)nio, key->gamma2,
          key->delta2, twist_b(), (flags & G16_VERIFY_SUBGROUP) ? 1u : 0u, (fp12_t*)(ws + o_mil),
          (int32_t*)(ws + o_st));
  KLAUNCH(ctx, "verify_final", verify_final, (uint32_t)((count + PBLOCK - 1) / PBLOCK), PBLOCK, 0,
          (const fp12_t*)(ws + o_mil), (const fp12_t*)key->d_ab.get(), (uint32_t)count, (int32_t*)(ws + o_st));
  HIPCHK(ctx, hipGetLastError());
  HIPCHK(ctx, hipMemcpyAsync(status, ws + o_st, count * 4, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return G16_OK;
}

extern "C" int32_t g16_verify_batch(g16_ctx* ctx, const g16_vkey* key, const g16_proof* proofs, const void* public_io,
                                    uint32_t flags, size_t count, const void* multipliers, int32_t* result,
                                    int32_t* status) {
  if (!ctx) return G16_EINVAL;
  if (!key || key->device != ctx->device || !result || (count && (!proofs || !public_io || !multipliers)) ||
      count >= (size_t(1) << 22)) {
    ctx->err = "g16_verify_batch: bad arguments";
    return G16_EINVAL;
  }
  for (size_t j = 0; j < count; ++j) {   // on the host, before anything is queued
    uint64_t z[2];
    memcpy(z, (const char*)multipliers + 16 * j, 16);
    if (!(z[0] | z[1])) {
      ctx->err = "g16_verify_batch: multiplier " + std::to_string(j) + " is zero";
      return G16_EINVAL;
    }
  }
  *result = 1;
  if (!count) return G16_OK;
  CTX_ENTER(ctx);
  const size_t nio = (size_t)key->npubs + 1, total = count * nio;
  const uint32_t nb = (uint32_t)((count + PBLOCK - 1) / PBLOCK), nbio = (uint32_t)((nio + PBLOCK - 1) / PBLOCK),
                 nbm = (uint32_t)((count + 3 + PBLOCK - 1) / PBLOCK);
  size_t o = 0;
  auto take = [&](size_t bytes) {
    size_t r = o;
    o += (bytes + 255) & ~size_t(255);
    return r;
  };
  const size_t o_pr = take(count * sizeof(g16_proof)), o_pub = take(total * 32), o_z = take(count * 16),
               o_bst = take(count * 4), o_s = take((nio + 1) * 32), o_nega = take(count * sizeof(g1_aff)),
               o_zc = take(count * sizeof(g1_acc)), o_icp = take(nio * sizeof(g1_acc)),
               o_fix = take(3 * sizeof(g1_aff)), o_gpart = take(2 * PBLOCK * sizeof(g1_acc)),
               o_mil = take((count + 3) * sizeof(fp12_t)), o_fpart = take((PBLOCK + 1) * sizeof(fp12_t)),
               o_res = take(4);
  // the per-proof path of g16_verify, run only for the statuses of a rejected batch
  const size_t o_part = status ? take(total * sizeof(g1_acc)) : 0, o_mil3 = status ? take(3 * count * sizeof(fp12_t)) : 0,
               o_st = status ? take(count * 4) : 0;
  int32_t rc;
  if ((rc = ensure(ctx, ctx->stage_p, o))) return rc;
  char* ws = (char*)ctx->stage_p.p();
  const uint32_t mont = (flags & G16_SCALARS_MONT) ? 1u : 0u;
  const g16_proof* d_pr = (const g16_proof*)(ws + o_pr);
  const uint4* d_z = (const uint4*)(ws + o_z);
  int32_t* d_bst = (int32_t*)(ws + o_bst);
  g1_aff* d_fix = (g1_aff*)(ws + o_fix);
  const char* ab = (const char*)key->d_ab.get();   // Miller value | alpha1 | beta2
  HIPCHK(ctx, hipMemcpyAsync(ws + o_pr, proofs, count * sizeof(g16_proof), hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(ws + o_pub, public_io, total * 32, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(ws + o_z, multipliers, count * 16, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipMemsetAsync(d_bst, 0, count * 4, ctx->stream));
  KLAUNCH(ctx, "batch_fold_pub", batch_fold_pub, (uint32_t)(nio + 1), PBLOCK, 0, (const u256*)(ws + o_pub), mont, d_z,
          (uint32_t)nio, (uint32_t)count, (u256*)(ws + o_s), d_bst);
  KLAUNCH(ctx, "batch_scale", batch_scale, 2 * nb + nbio + 1, PBLOCK, 0, d_pr, d_z, (uint32_t)count,
          (const u256*)(ws + o_s), (const g1_aff*)key->d_ic.get(), (uint32_t)nio,
          (const g1_aff*)(ab + sizeof(fp12_t)), twist_b(), (g1_aff*)(ws + o_nega), (g1_acc*)(ws + o_zc),
          (g1_acc*)(ws + o_icp), d_fix, d_bst);
  {
    g1_acc* gpart = (g1_acc*)(ws + o_gpart);
    G1Sum c{(const g1_acc*)(ws + o_zc), (uint32_t)count, d_bst, gpart, nullptr};
    G1Sum x{(const g1_acc*)(ws + o_icp), (uint32_t)nio, nullptr, gpart + PBLOCK, nullptr};
    const uint32_t g = std::min<uint32_t>(std::max(nb, nbio), PBLOCK);
    KLAUNCH(ctx, "batch_g1_sum", batch_g1_sum, dim3(g, 2), PBLOCK, 0, c, x);
    c = G1Sum{gpart, g, nullptr, nullptr, d_fix};
    x = G1Sum{gpart + PBLOCK, g, nullptr, nullptr, d_fix + 1};
    KLAUNCH(ctx, "batch_g1_sum", batch_g1_sum, dim3(1, 2), PBLOCK, 0, c, x);
  }
  KLAUNCH(ctx, "batch_miller", batch_miller, nbm + nb, PBLOCK, 0, d_pr, (uint32_t)count,
          (const g1_aff*)(ws + o_nega), (const g1_aff*)d_fix, key->delta2, key->gamma2,
          (const g2_aff*)(ab + sizeof(fp12_t) + 64), twist_b(), (fp12_t*)(ws + o_mil), d_bst);
  {
    fp12_t* fpart = (fp12_t*)(ws + o_fpart);
    const uint32_t g = std::min<uint32_t>(nbm, PBLOCK);
    KLAUNCH(ctx, "batch_gt_product", batch_gt_product, g, PBLOCK, 0, (const fp12_t*)(ws + o_mil),
            (uint32_t)(count + 3), (const int32_t*)d_bst, (uint32_t)count, fpart);
    KLAUNCH(ctx, "batch_gt_product", batch_gt_product, 1, PBLOCK, 0, (const fp12_t*)fpart, g,
            (const int32_t*)nullptr, 0u, fpart + PBLOCK);
    KLAUNCH(ctx, "batch_final", batch_final, 1, PBLOCK, 0, (const fp12_t*)(fpart + PBLOCK), (const int32_t*)d_bst,
            (uint32_t)count, (int32_t*)(ws + o_res));
  }
  HIPCHK(ctx, hipGetLastError());
  HIPCHK(ctx, hipMemcpyAsync(result, ws + o_res, 4, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  if (!status) return G16_OK;
  if (*result == 1) {
    for (size_t j = 0; j < count; ++j) status[j] = 1;
    return G16_OK;
  }
  // rejected: which proofs, by the per-proof kernels on the data already on the device
  HIPCHK(ctx, hipMemsetAsync(ws + o_st, 0, count * 4, ctx->stream));
  KLAUNCH(ctx, "verify_pub_terms", verify_pub_terms, (uint32_t)((total + PBLOCK - 1) / PBLOCK), PBLOCK, 0,
          (const u256*)(ws + o_pub), mont, (const g1_aff*)key->d_ic.get(), (uint32_t)nio, (uint32_t)total,
          (g1_acc*)(ws + o_part), (int32_t*)(ws + o_st));
  KLAUNCH(ctx, "verify_miller", verify_miller, (uint32_t)((3 * count + PBLOCK - 1) / PBLOCK), PBLOCK, 0, d_pr,
          (uint32_t)count, (const g1_acc*)(ws + o_part), (uint32_t)nio, key->gamma2, key->delta2, twist_b(), 1u,
          (fp12_t*)(ws + o_mil3), (int32_t*)(ws + o_st));
  KLAUNCH(ctx, "verify_final", verify_final, nb, PBLOCK, 0, (const fp12_t*)(ws + o_mil3),
          (const fp12_t*)key->d_ab.get(), (uint32_t)count, (int32_t*)(ws + o_st));
  HIPCHK(ctx, hipGetLastError());
  HIPCHK(ctx, hipMemcpyAsync(status, ws + o_st, count * 4, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return G16_OK;
}
