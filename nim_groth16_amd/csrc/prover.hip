// Proving-key residency and the per-proof launch sequence: the GPU counterpart of
// generateProofWithMask (reference groth16/prover.nim:215-304).
//   buildABC                      prover.nim:56-73     -> spmv_binned kernel (spmv.hip; rows binned once per key)
//   computeSnarkjsScalarCoeffs /  prover.nim:158-181   -> g16_quotient_device (ntt.hip)
//   computeQuotientPointwise      prover.nim:118-148
//   5 x msmMultiThreaded          prover.nim:282-302   -> msm_device on the registered point tables
//   mask algebra (`**`, `+=`)     prover.nim:279-302   -> O(1) curve operations on the host, as in the
//                                                         reference (curves.nim:136-214); not a hot loop
#include <algorithm>
#include <cstddef>
#include <new>

#include "g16_internal.hpp"
#include "b1_fold.cuh"
#include "host_curve.hpp"   // the host-side O(1) curve algebra of the combine step (ec.cuh, host_ff64.hpp)

using namespace g16;

// Immutable after g16_pkey_create and tied to a DEVICE, not to the creating context: the in-flight proofs of one
// GPU (one g16_ctx each: private streams and workspaces) all prove against ONE resident key, and the key may be
// destroyed before or after any of those contexts (ProverPoints are per-circuit constants, zkey_types.nim:36-41).
struct g16_pkey {
  int device = 0;
  uint32_t nvars = 0, npubs = 0, log2n = 0, flavour = 1;
  // this key holds the index ranges [lo, hi) of each point set (msm.nim:105-115 chunk rule over shard_count ranks)
  uint32_t shard_index = 0, shard_count = 1;
  size_t w_lo = 0, w_hi = 0;   // A1 / B1 / B2 / C1 : range of wires (C1 is stored wire-aligned, see below)
  size_t h_lo = 0, h_hi = 0;   // H1                : range of domain indices
  g16_points *A1 = nullptr, *B1 = nullptr, *B2 = nullptr, *C1 = nullptr, *H1 = nullptr;
  // the A and B matrices (zkey section 4 / ZKey.coeffs, zkey_types.nim:48-59), row-binned for buildABC (spmv.hip)
  g16_spmat* abc = nullptr;
  size_t ncoeffs = 0;
  g1_aff alpha1, beta1, delta1;
  g2_aff beta2, delta2;
  // Points at infinity.  snarkjs keys hold (0,0) in pointsA1 / pointsB1 / pointsB2 for every wire absent from the
  // matrix (the loaders accept them, curves.nim:95-107; the MSMs sum over them, msm.nim:128-158).  In the shared
  // witness sort such an entry still occupies a loop trip of a wave whose other lanes run a full addition, so a set
  // with >= G16_INF_COMPACT % of them gets entry lists of its own that leave them out: liveA = A1's bitmap, liveB =
  // the union of B1's and B2's (one sort serves both).  nullptr = dense: the set rides on the shared sort.
  const uint32_t* liveA = nullptr;   // not owned: A1's own bitmap
  DevMem<uint32_t> liveB;            // owned (the union), or empty
  size_t deadB = 0;               // wires whose B1 AND B2 points are both (0,0)
  // pointsB1 folded into pointsA1 (b1_fold_form, proof_plan.hpp).  B1_DELTA: `B1` holds the differences B1_i - A1_i
  // in place of pointsB1; B1_EMPTY: there is no live difference and the B1 accumulation runs against no table.  In both
  // the record's B1 slot holds MSM(w, difference) and the combine kernel adds the A1 slots to it.
  int b1_form = B1_PLAIN;
  size_t b1_inf = 0;              // (0,0) points of pointsB1 itself in this key's wire range
  size_t live_b1 = 0, live_delta = 0;   // over the WHOLE wire range: what the form was decided from
};

extern "C" void g16_pkey_destroy(g16_pkey* k) {
  if (!k) return;
  for (g16_points* p : {k->A1, k->B1, k->B2, k->C1, k->H1}) g16_points_release(p);
  // like g16_points_release: wait for the device, not for a context (the creating one may be gone already)
  (void)hipSetDevice(k->device);
  (void)hipDeviceSynchronize();
  g16_spmat_destroy(k->abc);
  delete k;   // (liveB goes with it)
}

// what the prover pool (pool.hip) needs to know about a key
void g16_pkey_shape(const g16_pkey* k, int* device, uint32_t* nvars, uint32_t* shard_count) {
  *device = k->device;
  *nvars = k->nvars;
  *shard_count = k->shard_count;
}

// points at infinity per set: out[0..4] = A1, B1, B2, C1 (without the public wires this library pads it with), H1;
// out[5] = wires whose B1 and B2 points are both (0,0); out[6] = 1 if A1, out[7] = 1 if B1/B2 use compacted entry lists
extern "C" int32_t g16_pkey_inf_counts(const g16_pkey* k, size_t out[8]) {
  if (!k || !out) return G16_EINVAL;
  // public wires 0 .. npubs of this shard's wire range: their C1 slots are this library's padding, not key points
  const size_t pub_end = std::min<size_t>(k->w_hi, (size_t)k->npubs + 1);
  const size_t pad = pub_end > k->w_lo ? pub_end - k->w_lo : 0;
  out[0] = k->A1->n_inf, out[1] = k->b1_inf, out[2] = k->B2->n_inf, out[3] = k->C1->n_inf - pad, out[4] = k->H1->n_inf;
  out[5] = k->deadB, out[6] = k->liveA ? 1 : 0, out[7] = k->liveB ? 1 : 0;
  return G16_OK;
}

// out[0] = the key's B1Form (0: pointsB1 as it is, 1: no live difference, 2: the differences in its place), out[1] =
// pointsB1 entries that are not (0,0), out[2] = wires whose pointsB1 and pointsA1 entries differ -- both counted over the
// whole wire range of the key, whichever shard this is
extern "C" int32_t g16_pkey_b1_fold(const g16_pkey* k, size_t out[3]) {
  if (!k || !out) return G16_EINVAL;
  out[0] = (size_t)k->b1_form, out[1] = k->live_b1, out[2] = k->live_delta;
  return G16_OK;
}

extern "C" int32_t g16_pkey_abc_info(const g16_pkey* k, size_t out[11]) {
  if (!k || !out) return G16_EINVAL;
  out[0] = k->ncoeffs;
  g16_spmat_info(k->abc, out + 1);
  return G16_OK;
}

// where a key's A / B coefficients come from: an array of g16_coeff (values c R), or the .zkey file's section 4 as it
// lies on disk (44-byte entries, values c R^2: files/zkey.nim:169-192, io.nim:134-139)
struct CoeffSource {
  const unsigned char* base = nullptr;   // first entry
  size_t count = 0, stride = 0, value_off = 0;
  bool values_r2 = false;
};
static inline uint32_t rd32(const unsigned char* p) {
  uint32_t v;
  memcpy(&v, p, 4);   // section 4 is not 4-byte aligned past its first entry
  return v;
}

// ---- pointsB1 against pointsA1 (key creation; b1_fold_form, proof_plan.hpp) --------------------------------------------
// cnt[0] += #{B1_i != (0,0)}, cnt[1] += #{B1_i != A1_i}: equality of the 64 bytes, which for the canonical encodings a key
// holds is equality of the points
static __global__ void __launch_bounds__(256) b1_compare_kernel(const uint4* __restrict__ a1, const uint4* __restrict__ b1,
                                                                uint32_t n, uint32_t* __restrict__ cnt) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  bool live = false, differs = false;
  if (i < n) {
    uint32_t any = 0, diff = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const uint4 a = a1[(size_t)i * 4 + q], b = b1[(size_t)i * 4 + q];
      any |= b.x | b.y | b.z | b.w;
      diff |= (a.x ^ b.x) | (a.y ^ b.y) | (a.z ^ b.z) | (a.w ^ b.w);
    }
    live = any != 0, differs = diff != 0;
  }
  const uint32_t nl = (uint32_t)__popcll(__ballot(live)), nd = (uint32_t)__popcll(__ballot(differs));
  if ((threadIdx.x & 63) == 0) {
    if (nl) atomicAdd(&cnt[0], nl);
    if (nd) atomicAdd(&cnt[1], nd);
  }
}
// b1[i] <- b1[i] - a1[i], exact and in the canonical affine form (b1_fold.cuh).  One thread per wire with an inversion of
// its own: this runs once per key.
static __global__ void __launch_bounds__(256) b1_delta_kernel(const g1_aff* __restrict__ a1, g1_aff* __restrict__ b1,
                                                              uint32_t n) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  b1[i] = point_difference<G1>(b1[i], a1[i]);
}

// table_stride: the stride of all five point sets (g16_points_register_*_lean; 0 / 1: a table per window)
static int32_t pkey_create(g16_ctx* ctx, const g16_pkey_desc* d, const CoeffSource& cs, uint32_t table_stride,
                           g16_pkey** out) {
  const size_t n = size_t(1) << d->log2_domain;
  // shape rules of generateProofWithMask (prover.nim:236, 270-276)
  if (d->log2_domain > 27 || d->nvars == 0 || d->npubs + 1 > d->nvars || d->flavour > 1 || !d->pointsA1 ||
      !d->pointsB1 || !d->pointsB2 || !d->pointsH1 || (d->nvars - d->npubs - 1 > 0 && !d->pointsC1) ||
      !d->alpha1 || !d->beta1 || !d->delta1 || !d->beta2 || !d->delta2) {
    ctx->err = "bad proving-key description";
    return G16_EINVAL;
  }
  CTX_ENTER(ctx);
  Building<g16_pkey, g16_pkey_destroy> k(new (std::nothrow) g16_pkey());
  if (!k) return G16_ENOMEM;
  k->device = ctx->device;
  k->nvars = d->nvars;
  k->npubs = d->npubs;
  k->log2n = d->log2_domain;
  k->flavour = d->flavour;
  memcpy(&k->alpha1, d->alpha1, 64);
  memcpy(&k->beta1, d->beta1, 64);
  memcpy(&k->delta1, d->delta1, 64);
  memcpy(&k->beta2, d->beta2, 128);
  memcpy(&k->delta2, d->delta2, 128);
  int32_t rc;
  // contiguous index ranges per rank: b = (N*(k+1)) div ntasks   (msm.nim:107-115)
  k->shard_count = d->shard_count ? d->shard_count : 1;
  k->shard_index = d->shard_index;
  if (k->shard_index >= k->shard_count) {
    ctx->err = "shard_index >= shard_count";
    return G16_EINVAL;
  }
  auto range = [&](size_t N, size_t& lo, size_t& hi) {
    lo = (N * k->shard_index) / k->shard_count;
    hi = (N * (k->shard_index + 1)) / k->shard_count;
  };
  range(d->nvars, k->w_lo, k->w_hi);
  range(n, k->h_lo, k->h_hi);
  // pointsC1 covers wires npubs+1 .. nvars-1 (zkey_types.nim:40; zs = witness[npubs+1..], prover.nim:262-264).
  // It is stored wire-aligned -- infinity for the npubs+1 public wires -- so that MSM(witness, C1') ==
  // MSM(zs, C1) and all four witness MSMs share ONE bucket arrangement of the witness.
  std::vector<unsigned char> c1pad((k->w_hi - k->w_lo) * 64, 0);
  for (size_t wI = k->w_lo; wI < k->w_hi; ++wI)
    if (wI > d->npubs) memcpy(&c1pad[(wI - k->w_lo) * 64], (const char*)d->pointsC1 + 64 * (wI - d->npubs - 1), 64);
  const uint32_t ts = table_stride;
  if ((rc = g16_points_register_g1_lean(ctx, (const char*)d->pointsA1 + 64 * k->w_lo, k->w_hi - k->w_lo, ts, &k->A1))) return rc;
  {   // pointsB1, or what stands in for it (b1_fold_form)
    const size_t nv = d->nvars, nw = k->w_hi - k->w_lo;
    SyncOnExit sync{ctx->stream};
    uint32_t cnt[2] = {0, 0};
    if (g16_env().b1_fold) {
      // the form is decided over every wire, whichever shard this is: the two whole arrays pass through a pair of small
      // buffers, a chunk at a time, so that the comparison costs a key no device memory worth speaking of
      constexpr size_t CHUNK = size_t(1) << 16;
      const size_t step = std::min(nv, CHUNK);
      DevMem<g1_aff> c_a1, c_b1;
      SyncOnExit sync_chunks{ctx->stream};
      if ((rc = ensure(ctx, ctx->stage_o, 2048))) return rc;
      uint32_t* d_cnt = (uint32_t*)ctx->stage_o.p();
      HIPCHK(ctx, dev_alloc(c_a1, step * sizeof(g1_aff)));
      HIPCHK(ctx, dev_alloc(c_b1, step * sizeof(g1_aff)));
      HIPCHK(ctx, hipMemsetAsync(d_cnt, 0, 8, ctx->stream));
      for (size_t lo = 0; lo < nv; lo += step) {
        const size_t m = std::min(step, nv - lo);
        HIPCHK(ctx, hipMemcpyAsync(c_a1.get(), (const char*)d->pointsA1 + 64 * lo, m * 64, hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(ctx, hipMemcpyAsync(c_b1.get(), (const char*)d->pointsB1 + 64 * lo, m * 64, hipMemcpyHostToDevice, ctx->stream));
        // (key creation: not a kernel of a proof, and not in the profile report)
        hipLaunchKernelGGL(b1_compare_kernel, dim3((uint32_t)((m + 255) / 256)), dim3(256), 0, ctx->stream,
                           (const uint4*)c_a1.get(), (const uint4*)c_b1.get(), (uint32_t)m, d_cnt);
        HIPCHK(ctx, hipGetLastError());
      }
      HIPCHK(ctx, hipMemcpyAsync(cnt, d_cnt, 8, hipMemcpyDeviceToHost, ctx->stream));
      HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    }
    k->live_b1 = cnt[0], k->live_delta = cnt[1];
    k->b1_form = b1_fold_form(cnt[0], cnt[1], nv, g16_env());
    if (k->b1_form == B1_DELTA && nw) {
      // this shard's range of the two arrays: the differences are built in place of the B1 points and registered from
      // the device (both arrays are gone before B2's tables are allocated)
      DevMem<g1_aff> d_a1, d_b1;
      SyncOnExit sync_arrays{ctx->stream};
      HIPCHK(ctx, dev_alloc(d_a1, nw * sizeof(g1_aff)));
      HIPCHK(ctx, dev_alloc(d_b1, nw * sizeof(g1_aff)));
      HIPCHK(ctx, hipMemcpyAsync(d_a1.get(), (const char*)d->pointsA1 + 64 * k->w_lo, nw * 64, hipMemcpyHostToDevice, ctx->stream));
      HIPCHK(ctx, hipMemcpyAsync(d_b1.get(), (const char*)d->pointsB1 + 64 * k->w_lo, nw * 64, hipMemcpyHostToDevice, ctx->stream));
      // (0,0) points of pointsB1 itself in this range, before the differences replace them
      uint32_t n_inf = 0;
      DevMem<uint32_t> scratch_live;
      uint32_t* d_cnt = (uint32_t*)ctx->stage_o.p();
      HIPCHK(ctx, dev_alloc(scratch_live, ((nw + 31) / 32 + 1) * 4));
      HIPCHK(ctx, hipMemsetAsync(d_cnt, 0, 4, ctx->stream));
      if ((rc = live_bitmap_device<G1>(ctx, d_b1.get(), nw, scratch_live.get(), d_cnt))) return rc;
      HIPCHK(ctx, hipMemcpyAsync(&n_inf, d_cnt, 4, hipMemcpyDeviceToHost, ctx->stream));
      hipLaunchKernelGGL(b1_delta_kernel, dim3((uint32_t)((nw + 255) / 256)), dim3(256), 0, ctx->stream,
                         (const g1_aff*)d_a1.get(), d_b1.get(), (uint32_t)nw);
      HIPCHK(ctx, hipGetLastError());
      HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
      k->b1_inf = n_inf;
      if ((rc = g16_points_register_g1_lean_dev(ctx, d_b1.get(), nw, ts, &k->B1))) return rc;
    } else {
      // B1_EMPTY keeps pointsB1 registered in full although no proof reads its tables (run_plan hands the B1 run no
      // table): the set still gives the key its B1 counts, bitmap and window configuration, and the reports of a key's
      // table bytes stay what they were.  That is memory and key-creation time spent for nothing on such a key.
      if ((rc = g16_points_register_g1_lean(ctx, (const char*)d->pointsB1 + 64 * k->w_lo, nw, ts, &k->B1))) return rc;
      k->b1_inf = k->B1->n_inf;
    }
  }
  if ((rc = g16_points_register_g2_lean(ctx, (const char*)d->pointsB2 + 128 * k->w_lo, k->w_hi - k->w_lo, ts, &k->B2))) return rc;
  if ((rc = g16_points_register_g1_lean(ctx, c1pad.data(), k->w_hi - k->w_lo, ts, &k->C1))) return rc;
  if ((rc = g16_points_register_g1_lean(ctx, (const char*)d->pointsH1 + 64 * k->h_lo, k->h_hi - k->h_lo, ts, &k->H1))) return rc;
  {   // sparse sets get their own entry lists (see g16_pkey)
    const size_t nw = k->w_hi - k->w_lo;
    k->liveA = g16_points_live_if_sparse(k->A1);
    if (nw && k->b1_form == B1_DELTA && k->B2->d_live) {
      // B1_i = (0,0) <=> B2_i = (0,0): the union of the two bitmaps is B2's own, and only B2 reads that arrangement
      k->deadB = k->B2->n_inf;
      if (points_sparse(k->deadB, nw, g16_env())) {
        const size_t words = (nw + 31) / 32 + 1;
        HIPCHK(ctx, dev_alloc(k->liveB, words * 4));
        HIPCHK(ctx, hipMemcpyAsync(k->liveB.get(), k->B2->d_live.get(), words * 4, hipMemcpyDeviceToDevice, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
      }
    } else if (nw && k->B1->d_live && k->B2->d_live) {
      uint32_t dead = 0;
      if ((rc = ensure(ctx, ctx->stage_o, 2048))) return rc;
      uint32_t* d_cnt = (uint32_t*)ctx->stage_o.p();
      HIPCHK(ctx, dev_alloc(k->liveB, ((nw + 31) / 32 + 1) * 4));
      HIPCHK(ctx, hipMemsetAsync(d_cnt, 0, 4, ctx->stream));
      if ((rc = g16_bitmap_or_device(ctx, k->liveB.get(), k->B1->d_live.get(), k->B2->d_live.get(), nw, d_cnt))) return rc;
      HIPCHK(ctx, hipMemcpyAsync(&dead, d_cnt, 4, hipMemcpyDeviceToHost, ctx->stream));
      HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
      k->deadB = dead;
      if (!points_sparse(dead, nw, g16_env())) k->liveB.reset();   // dense: share the witness sort
    }
  }
  // the A and B entries in row order, rows binned by length (sum order is irrelevant mod r)
  std::vector<uint32_t> vrow;
  try {
    vrow.resize(cs.count ? cs.count : 1);
  } catch (const std::bad_alloc&) {
    ctx->err = "out of host memory";
    return G16_ENOMEM;
  }
  for (size_t e = 0; e < cs.count; ++e) {
    const unsigned char* ent = cs.base + e * cs.stride;
    const uint32_t matrix = rd32(ent), row = rd32(ent + 4), col = rd32(ent + 8);
    if (matrix > 1 || row >= n || col >= d->nvars) {
      // MatrixC entries make the reference's buildABC raise (prover.nim:67)
      ctx->err = "coefficient entry out of range (matrix must be 0=A or 1=B)";
      return G16_EINVAL;
    }
    vrow[e] = 2 * row + matrix;
  }
  k->ncoeffs = cs.count;
  if ((rc = g16_spmat_create(ctx, 2, (uint32_t)n, cs.count, vrow.data(), 4, (const uint32_t*)(cs.count ? cs.base + 8 : nullptr),
                             cs.stride, cs.count ? cs.base + cs.value_off : nullptr, cs.stride, &k->abc, cs.values_r2)))
    return rc;
  *out = k.release();
  return G16_OK;
}

extern "C" int32_t g16_pkey_create_lean(g16_ctx* ctx, const g16_pkey_desc* d, uint32_t table_stride, g16_pkey** out) {
  if (!ctx) return G16_EINVAL;
  if (!d || !out || (d->ncoeffs && !d->coeffs)) {
    ctx->err = "null argument";
    return G16_EINVAL;
  }
  *out = nullptr;
  static_assert(sizeof(g16_coeff) == 48 && offsetof(g16_coeff, value) == 16, "g16_coeff layout");
  CoeffSource cs;
  cs.base = (const unsigned char*)d->coeffs, cs.count = d->ncoeffs, cs.stride = sizeof(g16_coeff), cs.value_off = 16;
  return pkey_create(ctx, d, cs, table_stride, out);
}
extern "C" int32_t g16_pkey_create(g16_ctx* ctx, const g16_pkey_desc* d, g16_pkey** out) {
  return g16_pkey_create_lean(ctx, d, 0, out);
}

// the key's coefficients straight from the .zkey file: section 4 as it lies on disk -- u32 count, then count entries of
// { u32 matrix, u32 row, u32 col, 32-byte value in DOUBLE Montgomery form } (files/zkey.nim:169-192; io.nim:134-139
// unmarshalFrWTF).  No host arithmetic: the values go to the device as they are.
extern "C" int32_t g16_pkey_create_zkey_lean(g16_ctx* ctx, const g16_pkey_desc* d, const void* section4,
                                             size_t section4_bytes, uint32_t table_stride, g16_pkey** out) {
  if (!ctx) return G16_EINVAL;
  if (!d || !out || !section4 || section4_bytes < 4 || d->coeffs || d->ncoeffs) {
    ctx->err = "bad argument (section 4 of the .zkey in, desc.coeffs = NULL, desc.ncoeffs = 0)";
    return G16_EINVAL;
  }
  *out = nullptr;
  const unsigned char* p = (const unsigned char*)section4;
  const size_t count = rd32(p);
  if (section4_bytes != 4 + count * 44) {
    ctx->err = "unexpected length of the coefficient section (4 + 44 * count bytes)";   // zkey.nim:176 asserts the same
    return G16_EINVAL;
  }
  CoeffSource cs;
  cs.base = p + 4, cs.count = count, cs.stride = 44, cs.value_off = 12, cs.values_r2 = true;
  return pkey_create(ctx, d, cs, table_stride, out);
}
extern "C" int32_t g16_pkey_create_zkey(g16_ctx* ctx, const g16_pkey_desc* d, const void* section4, size_t section4_bytes,
                                        g16_pkey** out) {
  return g16_pkey_create_zkey_lean(ctx, d, section4, section4_bytes, 0, out);
}

// Az | Bz | Cz for a witness (device buffers); exposed for tests of the buildABC kernel
// need_cz = false: only Az | Bz (Montgomery); the quotient forms Cz = Az * Bz while its first pass loads (ntt.cuh)
static int32_t build_abc_device(g16_ctx* ctx, const g16_pkey* k, const u256* d_wit, uint32_t wit_mont, u256* d_abc,
                                bool need_cz = true) {
  return g16_spmat_apply(ctx, k->abc, d_wit, wit_mont, d_abc, need_cz);
}

extern "C" int32_t g16_build_abc(g16_ctx* ctx, const g16_pkey* k, const void* witness, uint32_t flags, void* out_abc) {
  if (!ctx) return G16_EINVAL;
  if (!k || !witness || !out_abc || k->device != ctx->device) {
    ctx->err = "bad argument";
    return G16_EINVAL;
  }
  CTX_ENTER(ctx);
  const size_t n = size_t(1) << k->log2n;
  int32_t rc;
  if ((rc = ensure(ctx, ctx->prove, ((size_t)k->nvars + 4 * n) * 32))) return rc;
  u256* d_w = (u256*)ctx->prove.p();
  u256* d_abc = d_w + k->nvars;
  HIPCHK(ctx, hipMemcpyAsync(d_w, witness, (size_t)k->nvars * 32, hipMemcpyHostToDevice, ctx->stream));
  if ((rc = build_abc_device(ctx, k, d_w, (flags & G16_SCALARS_MONT) ? 1u : 0u, d_abc))) return rc;
  HIPCHK(ctx, hipMemcpyAsync(out_abc, d_abc, 3 * n * 32, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return G16_OK;
}

// record of the five MSM partials of one rank: XYZZ accumulators (Montgomery), fixed order
//   [0,128) A1 | [128,256) B1 | [256,512) B2 (G2) | [512,640) H1 | [640,768) C1
static constexpr size_t PART_A = 0, PART_B1 = 128, PART_B2 = 256, PART_H = 512, PART_C = 640, PART_BYTES = 768;

// ---- a proof's launch sequence: the plan (proof_plan.hpp) decides, run_plan issues ------------------------------
static ProofShape proof_shape(const g16_pkey* k) {
  return ProofShape{k->w_hi - k->w_lo, k->h_hi - k->h_lo, k->log2n, k->liveA != nullptr, (bool)k->liveB,
                    k->C1->cfg() == k->H1->cfg(), k->b1_form};
}

// what the steps of one entry point work on
struct ProofArgs {
  const void* witness = nullptr;   // (whole proof, _begin)
  uint32_t flags = 0;
  u256* task_out = nullptr;        // _begin: the coset vectors, n Fr each
  const void *d_a1 = nullptr, *d_b1 = nullptr, *d_c1 = nullptr;   // _end: this key's slices of them
  bool qs_is_slice = false;        // _end: the H scalars lie at the start of the qs buffer, not at h_lo
  void* out_partials = nullptr;
};

static int32_t run_plan(g16_ctx* ctx, const g16_pkey* k, ProofEntry entry, uint32_t task_mask, bool host_sync,
                        const ProofArgs& a) {
  ProofPlan plan;
  if (!proof_plan_build(plan, g16_env(), entry, task_mask, host_sync, proof_shape(k))) {
    ctx->err = "proof launch plan exceeds its capacity";
    return G16_EINVAL;
  }
  const size_t n = size_t(1) << k->log2n, nw = k->w_hi - k->w_lo, nh = k->h_hi - k->h_lo;
  int32_t rc;
  if ((rc = ensure(ctx, ctx->prove, ((size_t)k->nvars + 4 * n) * 32))) return rc;
  if ((rc = ensure(ctx, ctx->stage_o, 2048))) return rc;
  u256* const d_w = (u256*)ctx->prove.p();   // per-proof scalars: witness | Az | Bz | Cz | qs
  u256* const d_abc = d_w + k->nvars;
  u256* const d_qs = d_abc + 3 * n;
  char* const slots = (char*)ctx->stage_o.p();
  const u256* const d_wr = d_w + k->w_lo;
  const u256* const d_qs_slice = a.qs_is_slice ? d_qs : d_qs + k->h_lo;   // the H scalars of [h_lo, h_hi), Montgomery
  const uint32_t wit_mont = (a.flags & G16_SCALARS_MONT) ? 1u : 0u;
  g16_ctx::MsmLane* L = ctx->lane;
  // the five MSMs (ProofRun order): arrangement, workspace, tables, slot of the record
  const g16_points* const sets[RUN_COUNT] = {k->A1, k->B1, k->C1, k->B2, k->H1};
  g16_msm_run runs[RUN_COUNT] = {
      {&ctx->sort[plan.sort_a], &L[0].acc, k->A1->d_tables.get(), nullptr, slots + PART_A, nullptr},
      // (B1_EMPTY: no table -- msm_accum leaves infinity in every bucket and the tail kernels take their early-outs)
      {&ctx->sort[plan.sort_b1], &L[2].acc, k->b1_form == B1_EMPTY ? nullptr : k->B1->d_tables.get(), nullptr,
       slots + PART_B1, nullptr},
      {&ctx->sort[SORT_W], &L[3].acc, k->C1->d_tables.get(), nullptr, slots + PART_C, nullptr},
      {&ctx->sort[plan.sort_b], &L[1].acc, k->B2->d_tables.get(), nullptr, slots + PART_B2, nullptr},
      {&ctx->sort[SORT_H], &L[4].acc, k->H1->d_tables.get(), nullptr, slots + PART_H, nullptr}};
  auto event = [&](int e) { return e == EV_NONE ? nullptr : e < EV_COUNT ? ctx->ev[e].get() : L[e - EV_DONE0].done.get(); };
  for (int i = 0; i < plan.count; ++i) {
    const ProofStep& s = plan.steps[i];
    rc = G16_OK;
    hipStream_t st = s.stream == PS_MAIN ? ctx->stream : L[s.stream].stream.get();
    switch (s.op) {
      case OP_UPLOAD:
        HIPCHK(ctx, hipMemcpyAsync(d_w, a.witness, (size_t)k->nvars * 32,
                                   (a.flags & G16_SCALARS_DEVICE) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
        HIPCHK(ctx, hipMemsetAsync(slots, 0, PART_BYTES, st));   // empty range -> XYZZ infinity (all zero)
        break;
      case OP_WAIT: HIPCHK(ctx, hipStreamWaitEvent(st, event(s.a), 0)); break;
      case OP_RECORD: HIPCHK(ctx, hipEventRecord(event(s.a), st)); break;
      case OP_SORT_W:
        ctx->sort[s.a].narrow_tail = plan.narrow_tail;
        rc = g16_msm_sort(ctx, st, d_wr, wit_mont ? G16_SCALARS_MONT : 0u, nw, sets[s.c]->cfg(), ctx->sort[s.a],
                          s.b == 0 ? nullptr : s.b == 1 ? k->liveA : k->liveB.get());
        break;
      case OP_SORT_H:
        ctx->sort[SORT_H].narrow_tail = plan.narrow_tail;
        rc = g16_msm_sort(ctx, st, d_qs_slice, G16_SCALARS_MONT, nh, k->H1->cfg(), ctx->sort[SORT_H]);
        break;
      case OP_BUILD_ABC: rc = build_abc_device(ctx, k, d_w, wit_mont, d_abc, s.a != 0); break;
      case OP_QUOTIENT:
        rc = g16_quotient_device(ctx, d_abc, d_abc + n, d_abc + 2 * n, k->log2n, (int)k->flavour, d_qs, s.a);
        break;
      case OP_COSET: {   // (the outputs of the set bits of task_mask lie one after the other)
        const int at = __builtin_popcount(task_mask & ((1u << s.a) - 1));
        rc = g16_coset_pipeline_device(ctx, d_abc + s.a * n, k->log2n, a.task_out + at * n);
        break;
      }
      case OP_POINTWISE: rc = g16_abc_pointwise_device(ctx, a.d_a1, a.d_b1, a.d_c1, nh, d_qs); break;
      case OP_MSM:
        runs[RUN_H].init_partial = s.e ? g16_msm_partial_ptr(L[3].acc) : nullptr;   // (read by H's step alone)
        rc = g16_msm_batch(ctx, st, s.a == RUN_B2 ? 2 : 1, &runs[s.a], s.b, s.c, event(s.d));
        break;
      case OP_COPY_OUT:
        HIPCHK(ctx, hipMemcpyAsync(a.out_partials, slots, PART_BYTES,
                                   (a.flags & G16_OUT_DEVICE) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, st));
        break;
      case OP_HOST_SYNC: HIPCHK(ctx, hipStreamSynchronize(st)); break;
    }
    if (rc) return rc;
  }
  return G16_OK;
}

extern "C" int32_t g16_prove_partials(g16_ctx* ctx, const g16_pkey* k, const void* witness, uint32_t flags,
                                      void* out_partials) {
  if (!ctx) return G16_EINVAL;
  if (!k || !witness || !out_partials || k->device != ctx->device) {
    ctx->err = "bad argument";
    return G16_EINVAL;
  }
  CTX_ENTER(ctx);
  ProofArgs a;
  a.witness = witness, a.flags = flags, a.out_partials = out_partials;
  // G16_NO_HOST_SYNC (device output only): the record is complete in stream order; the caller's next operation on
  // the context's stream (an all-gather enqueued on it, g16_prove_combine) is ordered behind it without a host wait
  const bool host_sync = !((flags & G16_NO_HOST_SYNC) && (flags & G16_OUT_DEVICE));
  const int32_t rc = run_plan(ctx, k, PROOF_WHOLE, 0, host_sync, a);
  // an error exit may leave work queued on the lane streams (e.g. a failed allocation after the witness MSMs were
  // launched): drain all of them before returning, so that the caller -- or the next call's ensure() -- can never
  // free a buffer a lane kernel is still reading
  if (rc != G16_OK) ctx_quiesce(ctx);
  return rc;
}

// ---- sharded proof with a task-parallel quotient ------------------------------------------------------------
// The reference runs the three coset pipelines of computeSnarkjsScalarCoeffs as three tasks (prover.nim:167-169).
// Across GPUs each pipeline lives on ONE rank: _begin launches this rank's witness MSMs and computes the pipelines
// named by task_mask (bit 0: A, bit 1: B, bit 2: C) into d_task_out (n Fr per set bit, ascending); the caller
// scatters the [h_lo, h_hi) slices of the three coset vectors to their ranks (nim_groth16_amd/distributed.py: three
// scatters of 32 n / G bytes per destination) while the MSM lanes keep computing; _end forms this rank's H scalars
// A1*B1 - C1 from the received slices (prover.nim:175-176), runs the H MSM over them and hands out the partials.
extern "C" int32_t g16_prove_partials_begin(g16_ctx* ctx, const g16_pkey* k, const void* witness, uint32_t flags,
                                            uint32_t task_mask, void* d_task_out) {
  if (!ctx) return G16_EINVAL;
  if (!k || !witness || k->device != ctx->device || task_mask > 7 || (task_mask && !d_task_out)) {
    ctx->err = "bad argument";
    return G16_EINVAL;
  }
  if (k->flavour != G16_FLAVOUR_SNARKJS) {
    ctx->err = "the task-parallel quotient serves snarkjs-flavour keys (JensGroth needs a 7th transform of the whole "
               "vector: use g16_prove_partials)";
    return G16_EINVAL;
  }
  CTX_ENTER(ctx);
  ProofArgs a;
  a.witness = witness, a.flags = flags, a.task_out = (u256*)d_task_out;
  const int32_t rc = run_plan(ctx, k, PROOF_BEGIN, task_mask, !(flags & G16_NO_HOST_SYNC), a);
  if (rc != G16_OK) {
    ctx_quiesce(ctx);
    return rc;
  }
  ctx->shard_begun = k;
  return G16_OK;
}

extern "C" int32_t g16_prove_partials_end(g16_ctx* ctx, const g16_pkey* k, const void* d_a1, const void* d_b1,
                                          const void* d_c1, uint32_t flags, void* out_partials) {
  if (!ctx) return G16_EINVAL;
  const size_t nh = k ? k->h_hi - k->h_lo : 0;
  if (!k || !out_partials || k->device != ctx->device || (nh && (!d_a1 || !d_b1 || !d_c1))) {
    ctx->err = "bad argument";
    return G16_EINVAL;
  }
  if (ctx->shard_begun != k) {
    ctx->err = "g16_prove_partials_end without a matching g16_prove_partials_begin on this context";
    return G16_EINVAL;
  }
  CTX_ENTER_KEEP(ctx);
  ctx->shard_begun = nullptr;
  ProofArgs a;
  a.flags = flags, a.d_a1 = d_a1, a.d_b1 = d_b1, a.d_c1 = d_c1, a.qs_is_slice = true, a.out_partials = out_partials;
  const int32_t rc = run_plan(ctx, k, PROOF_END, 0, !((flags & G16_NO_HOST_SYNC) && (flags & G16_OUT_DEVICE)), a);
  if (rc != G16_OK) ctx_quiesce(ctx);
  return rc;
}

// one workgroup per MSM: res = sum over ranks of that MSM's partial, then canonical affine
// (`res += sync pending[k]`, msm.nim:117-119, across GPUs instead of threads)
// fold_b1: the B1 slots hold MSM(w, B1 - A1) (a key with pointsB1 folded into pointsA1): B1 = the A1 slots + the B1 slots
static __global__ void prove_combine_kernel(const unsigned char* __restrict__ gathered, uint32_t count, uint32_t fold_b1,
                                            unsigned char* __restrict__ out) {
  if (threadIdx.x != 0) return;
  const uint32_t b = blockIdx.x;
  if (b == 2) {
    g2_acc r = G2::acc_inf();
    for (uint32_t i = 0; i < count; ++i) G2::add(r, *(const g2_acc*)(gathered + (size_t)i * PART_BYTES + PART_B2));
    *(g2_aff*)(out + 128) = G2::to_affine(r);
  } else {
    const size_t src = b == 0 ? PART_A : b == 1 ? PART_B1 : b == 3 ? PART_H : PART_C;
    const size_t dst = b == 0 ? 0 : b == 1 ? 64 : b == 3 ? 256 : 320;
    g1_acc r = G1::acc_inf();
    for (uint32_t i = 0; i < count; ++i) G1::add(r, *(const g1_acc*)(gathered + (size_t)i * PART_BYTES + src));
    if (b == 1 && fold_b1)
      for (uint32_t i = 0; i < count; ++i) G1::add(r, *(const g1_acc*)(gathered + (size_t)i * PART_BYTES + PART_A));
    *(g1_aff*)(out + dst) = G1::to_affine(r);
  }
}

// g16_prove_combine in two halves, shared with the prover pool (pool.hip).
// Enqueue half: stage copy + prove_combine_kernel on the context's main stream, the host algebra that needs only the
// mask and the key, then the copy of the five affine MSM sums (384 bytes) into `res_host` and, if `done` is given, an
// event behind it.  Into pageable memory the copy makes the host wait for the stream; into pinned memory it does not.
static_assert(sizeof(CombineRes) == G16_COMBINE_RES_BYTES, "slot layout");
static_assert(sizeof(CombinePre) == sizeof(g16_combine_pre), "g16_combine_pre layout");

int32_t g16_combine_enqueue(g16_ctx* ctx, const g16_pkey* k, const void* partials, size_t count, uint32_t flags,
                            const void* mask_r, const void* mask_s, void* res_host, hipEvent_t done,
                            g16_combine_pre* pre_out) {
  int32_t rc;
  if ((rc = ensure(ctx, ctx->stage_p, count * PART_BYTES))) return rc;
  if ((rc = ensure(ctx, ctx->stage_o, 2048))) return rc;
  HIPCHK(ctx, hipMemcpyAsync(ctx->stage_p.p(), partials, count * PART_BYTES,
                             (flags & G16_SCALARS_DEVICE) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice,
                             ctx->stream));
  unsigned char* d_res = (unsigned char*)ctx->stage_o.p() + 1024;
  KLAUNCH(ctx, "prove_combine", prove_combine_kernel, 5, 64, 0, (const unsigned char*)ctx->stage_p.p(), (uint32_t)count,
          k->b1_form != B1_PLAIN ? 1u : 0u, d_res);

  // Everything that depends on the mask and the key alone is computed while the GPU works -- in g16_prove that is the
  // whole proof, which is enqueued without a host wait (host_curve.hpp: host_combine_pre)
  u256 r = Fr::zero(), s = Fr::zero();
  if (mask_r) memcpy(&r, mask_r, 32);
  if (mask_s) memcpy(&s, mask_s, 32);
  const CombinePre pre = host_combine_pre(k->alpha1, k->beta1, k->delta1, k->beta2, k->delta2, r, s);
  memcpy(pre_out, &pre, sizeof pre);
  // (a copy into pageable host memory makes the host wait for the stream: it comes AFTER the host arithmetic above)
  HIPCHK(ctx, hipMemcpyAsync(res_host, d_res, sizeof(CombineRes), hipMemcpyDeviceToHost, ctx->stream));
  if (done) HIPCHK(ctx, hipEventRecord(done, ctx->stream));
  return G16_OK;
}

// Finish half: what needs the MSM results -- three additions and ONE joint double-scalar multiplication.  `res_host`
// must be complete (the stream or the enqueue half's event has passed the copy).
void g16_combine_finish(const g16_combine_pre* pre_in, const void* res_host, g16_proof* out) {
  CombinePre pre;
  CombineRes res;
  memcpy(&pre, pre_in, sizeof pre);
  memcpy(&res, res_host, sizeof res);
  g1_aff pi_a, pi_c;
  g2_aff pi_b;
  host_combine_finish(pre, res, pi_a, pi_b, pi_c);
  memcpy(out->pi_a, &pi_a, 64);
  memcpy(out->pi_b, &pi_b, 128);
  memcpy(out->pi_c, &pi_c, 64);
}

extern "C" int32_t g16_prove_combine(g16_ctx* ctx, const g16_pkey* k, const void* partials, size_t count,
                                     uint32_t flags, const void* mask_r, const void* mask_s, g16_proof* out) {
  if (!ctx) return G16_EINVAL;
  if (!k || !partials || !out || k->device != ctx->device || count == 0 || count > 1024) {
    ctx->err = "bad argument";
    return G16_EINVAL;
  }
  CTX_ENTER(ctx);
  int32_t rc;
  CombineRes res;
  g16_combine_pre pre;
  if ((rc = g16_combine_enqueue(ctx, k, partials, count, flags, mask_r, mask_s, &res, nullptr, &pre))) return rc;
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  g16_combine_finish(&pre, &res, out);
  return G16_OK;
}

extern "C" int32_t g16_prove(g16_ctx* ctx, const g16_pkey* k, const void* witness, uint32_t flags, const void* mask_r,
                             const void* mask_s, g16_proof* out) {
  if (!ctx) return G16_EINVAL;
  if (!k || !witness || !out || k->device != ctx->device) {
    ctx->err = "bad argument";
    return G16_EINVAL;
  }
  if (k->shard_count != 1) {
    ctx->err = "g16_prove needs an unsharded key; use g16_prove_partials + g16_prove_combine";
    return G16_EINVAL;
  }
  CTX_ENTER(ctx);   // before the first allocation: a fresh host thread's current device is 0, not the context's
  int32_t rc;
  if ((rc = ensure(ctx, ctx->stage_o, 2048))) return rc;
  if ((rc = ensure(ctx, ctx->stage_s, PART_BYTES))) return rc;
  // partials stay in HBM (stage_s is free again once the witness has been copied into the prove buffer)
  unsigned char* d_part = (unsigned char*)ctx->stage_s.p();
  // no host wait here: the combine's copy and kernel are ordered behind the record on the main stream, and its
  // mask-only host arithmetic (~0.3 ms) then overlaps the whole proof instead of following it
  if ((rc = g16_prove_partials(ctx, k, witness, flags | G16_OUT_DEVICE | G16_NO_HOST_SYNC, d_part))) return rc;
  rc = g16_prove_combine(ctx, k, d_part, 1, G16_SCALARS_DEVICE, mask_r, mask_s, out);
  if (rc != G16_OK) ctx_quiesce(ctx);   // a failed combine may leave the lanes running
  return rc;
}

// quotient alone, host pointers (replaces computeSnarkjsScalarCoeffs / computeQuotientPointwise)
extern "C" int32_t g16_quotient(g16_ctx* ctx, const void* Az, const void* Bz, const void* Cz, uint32_t log2n,
                                uint32_t flavour, void* out) {
  if (!ctx) return G16_EINVAL;
  if (!Az || !Bz || !Cz || !out || log2n > 27 || flavour > 1) {
    ctx->err = "bad argument";
    return G16_EINVAL;
  }
  CTX_ENTER(ctx);
  const size_t n = size_t(1) << log2n;
  int32_t rc;
  if ((rc = ensure(ctx, ctx->prove, 4 * n * 32))) return rc;
  u256* d = (u256*)ctx->prove.p();
  HIPCHK(ctx, hipMemcpyAsync(d, Az, n * 32, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(d + n, Bz, n * 32, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(d + 2 * n, Cz, n * 32, hipMemcpyHostToDevice, ctx->stream));
  if ((rc = g16_quotient_device(ctx, d, d + n, d + 2 * n, log2n, (int)flavour, d + 3 * n))) return rc;
  HIPCHK(ctx, hipMemcpyAsync(out, d + 3 * n, n * 32, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return G16_OK;
}
extern "C" int32_t g16_quotient_dev(g16_ctx* ctx, const void* d_Az, const void* d_Bz, const void* d_Cz, uint32_t log2n,
                                    uint32_t flavour, void* d_out) {
  if (!ctx) return G16_EINVAL;
  if (!d_Az || !d_Bz || !d_Cz || !d_out || log2n > 27 || flavour > 1) {
    ctx->err = "bad argument";
    return G16_EINVAL;
  }
  CTX_ENTER(ctx);
  return g16_quotient_device(ctx, d_Az, d_Bz, d_Cz, log2n, (int)flavour, d_out);
}
