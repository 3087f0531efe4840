// Proving-key residency: what g16_pkey_create* leaves on the device for the proofs of prover.hip, and what a key
// reports about itself.  The rules -- which indices a shard holds, the padding of C1, the form pointsB1 takes, where the
// entry lists of the B sets come from -- are key_plan.hpp's; the steps below carry them out, each with its own
// temporaries and its own drain before they are freed.
#include <algorithm>
#include <cstddef>
#include <new>

#include "pkey.hpp"
#include "b1_fold.cuh"

using namespace g16;

extern "C" void g16_pkey_destroy(g16_pkey* k) {
  if (!k) return;
  for (g16_points* p : {k->A1, k->B1, k->B2, k->C1, k->H1}) g16_points_release(p);
  // like g16_points_release: wait for the device, not for a context (the creating one may be gone already)
  (void)hipSetDevice(k->device);
  (void)hipDeviceSynchronize();
  g16_spmat_destroy(k->abc);
  delete k;   // (liveB goes with it)
}

// points at infinity per set: out[0..4] = A1, B1, B2, C1 (without the public wires this library pads it with), H1;
// out[5] = wires whose B1 and B2 points are both (0,0); out[6] = 1 if A1, out[7] = 1 if B1/B2 use compacted entry lists
extern "C" int32_t g16_pkey_inf_counts(const g16_pkey* k, size_t out[8]) {
  if (!k || !out) return G16_EINVAL;
  out[0] = k->A1->n_inf, out[1] = k->b1_inf, out[2] = k->B2->n_inf, out[4] = k->H1->n_inf;
  out[3] = k->C1->n_inf - c1_padding(k->w, k->npubs);
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

// out[0] = 1 if the key's B1 job takes the sparse run (a DELTA key with at most out[2] = B1_SPARSE_MAX live differences
// over its whole wire range), out[1] = the live differences in THIS key's wire range
extern "C" int32_t g16_pkey_b1_sparse(const g16_pkey* k, size_t out[3]) {
  if (!k || !out) return G16_EINVAL;
  out[0] = k->b1_sparse ? 1 : 0, out[1] = k->b1_nlive, out[2] = B1_SPARSE_MAX;
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

// ---- pointsB1 against pointsA1 (b1_fold_form, key_plan.hpp) ------------------------------------------------------------
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

// ---- the steps of key creation, in order ---------------------------------------------------------------------------------
// shape rules of generateProofWithMask (prover.nim:236, 270-276)
static bool desc_well_formed(const g16_pkey_desc* d) {
  return d->log2_domain <= 27 && d->nvars != 0 && d->npubs + 1 <= d->nvars && d->flavour <= 1 && d->pointsA1 &&
         d->pointsB1 && d->pointsB2 && d->pointsH1 && (d->nvars - d->npubs - 1 == 0 || d->pointsC1) && d->alpha1 &&
         d->beta1 && d->delta1 && d->beta2 && d->delta2;
}

// 1. what the key is and which index ranges this shard of it holds
static int32_t key_layout(g16_ctx* ctx, const g16_pkey_desc* d, g16_pkey* k) {
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
  k->shard_count = d->shard_count ? d->shard_count : 1;
  k->shard_index = d->shard_index;
  if (k->shard_index >= k->shard_count) {
    ctx->err = "shard_index >= shard_count";
    return G16_EINVAL;
  }
  k->w = shard_range(d->nvars, k->shard_index, k->shard_count);
  k->h = shard_range(size_t(1) << d->log2_domain, k->shard_index, k->shard_count);
  return G16_OK;
}

// 2. the form pointsB1 takes.  It is decided over every wire, whichever shard this is: the two whole arrays pass through
// a pair of small buffers, a chunk at a time, so that the comparison costs a key no device memory worth speaking of
static int32_t b1_form_of_whole_arrays(g16_ctx* ctx, const g16_pkey_desc* d, g16_pkey* k) {
  const size_t nv = d->nvars;
  uint32_t cnt[2] = {0, 0};
  if (g16_env().b1_fold) {
    constexpr size_t CHUNK = size_t(1) << 16;
    const size_t step = std::min(nv, CHUNK);
    DevMem<g1_aff> c_a1, c_b1;
    SyncOnExit sync{ctx->stream};
    HIPCHK(ctx, dev_alloc(c_a1, step * sizeof(g1_aff)));
    HIPCHK(ctx, dev_alloc(c_b1, step * sizeof(g1_aff)));
    const int32_t rc = counted_launch(ctx, 0, cnt, 2, [&](uint32_t* d_cnt) -> int32_t {
      for (size_t lo = 0; lo < nv; lo += step) {
        const size_t m = std::min(step, nv - lo);
        HIPCHK(ctx, hipMemcpyAsync(c_a1.get(), (const char*)d->pointsA1 + 64 * lo, m * 64, hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(ctx, hipMemcpyAsync(c_b1.get(), (const char*)d->pointsB1 + 64 * lo, m * 64, hipMemcpyHostToDevice, ctx->stream));
        // (key creation: not a kernel of a proof, and not in the profile report)
        hipLaunchKernelGGL(b1_compare_kernel, dim3((uint32_t)((m + 255) / 256)), dim3(256), 0, ctx->stream,
                           (const uint4*)c_a1.get(), (const uint4*)c_b1.get(), (uint32_t)m, d_cnt);
        HIPCHK(ctx, hipGetLastError());
      }
      return G16_OK;
    });
    if (rc) return rc;
  }
  k->live_b1 = cnt[0], k->live_delta = cnt[1];
  k->b1_form = b1_fold_form(cnt[0], cnt[1], nv, g16_env());
  return G16_OK;
}

// ... and, for a DELTA key with few enough live differences (b1_sparse_run: the whole-range count decides for every
// shard), the live wires of this shard's range, read off the bitmap the registration of D has just made.  A shard whose
// range holds none keeps an empty list: its sparse run writes infinity throughout.
static int32_t b1_live_wires(g16_ctx* ctx, g16_pkey* k) {
  if (!b1_sparse_run(k->live_delta)) return G16_OK;
  const size_t nw = k->w.size(), words = (nw + 31) / 32;
  std::vector<uint32_t> bitmap(words), list(g16_pkey::B1_VIEW_WORDS, 0u);
  HIPCHK(ctx, hipMemcpyAsync(bitmap.data(), k->B1->d_live.get(), words * 4, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  for (size_t i = 0; i < nw; ++i)
    if ((bitmap[i >> 5] >> (i & 31)) & 1u) list.push_back((uint32_t)i);
  const size_t nlive = list.size() - g16_pkey::B1_VIEW_WORDS;
  if (nlive > B1_SPARSE_MAX || nlive != nw - k->B1->n_inf) {
    ctx->err = "the live differences of pointsB1 do not match their count";
    return G16_EINVAL;
  }
  list.push_back(0u);   // (an empty list still has an address)
  HIPCHK(ctx, dev_alloc(k->b1_sparse, list.size() * 4));
  HIPCHK(ctx, hipMemcpyAsync(k->b1_sparse.get(), list.data(), list.size() * 4, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  k->b1_nlive = (uint32_t)nlive;
  return G16_OK;
}

// 3. pointsB1 of this shard's wires, or what stands in for it
static int32_t register_b1(g16_ctx* ctx, const g16_pkey_desc* d, uint32_t table_stride, g16_pkey* k) {
  const size_t nw = k->w.size();
  int32_t rc;
  if (k->b1_form != B1_DELTA || !nw) {
    // B1_EMPTY keeps pointsB1 registered in full although no proof reads its tables (run_plan hands the B1 run no
    // table): the set still gives the key its B1 counts, bitmap and window configuration, and the reports of a key's
    // table bytes stay what they were.  That is memory and key-creation time spent for nothing on such a key.
    if ((rc = g16_points_register_g1_lean(ctx, (const char*)d->pointsB1 + 64 * k->w.lo, nw, table_stride, &k->B1))) return rc;
    k->b1_inf = k->B1->n_inf;
    return G16_OK;
  }
  // this shard's range of the two arrays: the differences are built in place of the B1 points and registered from
  // the device (both arrays are gone before B2's tables are allocated)
  DevMem<g1_aff> d_a1, d_b1;
  DevMem<uint32_t> scratch_live;
  SyncOnExit sync{ctx->stream};
  HIPCHK(ctx, dev_alloc(d_a1, nw * sizeof(g1_aff)));
  HIPCHK(ctx, dev_alloc(d_b1, nw * sizeof(g1_aff)));
  HIPCHK(ctx, hipMemcpyAsync(d_a1.get(), (const char*)d->pointsA1 + 64 * k->w.lo, nw * 64, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(d_b1.get(), (const char*)d->pointsB1 + 64 * k->w.lo, nw * 64, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, dev_alloc(scratch_live, ((nw + 31) / 32 + 1) * 4));
  // the (0,0) points of pointsB1 itself are counted before the differences replace them
  uint32_t n_inf = 0;
  rc = counted_launch(ctx, 0, &n_inf, 1, [&](uint32_t* d_n_inf) -> int32_t {
    if (int32_t e = live_bitmap_device<G1>(ctx, d_b1.get(), nw, scratch_live.get(), d_n_inf)) return e;
    hipLaunchKernelGGL(b1_delta_kernel, dim3((uint32_t)((nw + 255) / 256)), dim3(256), 0, ctx->stream,
                       (const g1_aff*)d_a1.get(), d_b1.get(), (uint32_t)nw);
    HIPCHK(ctx, hipGetLastError());
    return G16_OK;
  });
  if (rc) return rc;
  k->b1_inf = n_inf;
  if ((rc = g16_points_register_g1_lean_dev(ctx, d_b1.get(), nw, table_stride, &k->B1))) return rc;
  return b1_live_wires(ctx, k);
}

// pointsC1 covers wires npubs+1 .. nvars-1 (zkey_types.nim:40; zs = witness[npubs+1..], prover.nim:262-264).
// It is stored wire-aligned -- infinity for the npubs+1 public wires (c1_padding, key_plan.hpp) -- so that
// MSM(witness, C1') == MSM(zs, C1) and all four witness MSMs share ONE bucket arrangement of the witness.  The buffer
// is the host's largest temporary and is built before any device work: built between two registrations, measured, it
// costs key creation 2 to 15 % (profiles/key_creation_refactor_2p20.txt).
static std::vector<unsigned char> c1_wire_aligned(const g16_pkey_desc* d, const g16_pkey* k) {
  std::vector<unsigned char> c1pad(k->w.size() * 64, 0);
  for (size_t wI = k->w.lo + c1_padding(k->w, d->npubs); wI < k->w.hi; ++wI)
    memcpy(&c1pad[(wI - k->w.lo) * 64], (const char*)d->pointsC1 + 64 * (wI - d->npubs - 1), 64);
  return c1pad;
}

// 4. sparse sets get their own entry lists (see g16_pkey; live_b_source, key_plan.hpp)
static int32_t live_lists(g16_ctx* ctx, g16_pkey* k) {
  const size_t nw = k->w.size(), bitmap_bytes = ((nw + 31) / 32 + 1) * 4;
  k->liveA = g16_points_live_if_sparse(k->A1);
  const LiveSource source = live_b_source(k->b1_form, nw, (bool)k->B1->d_live, (bool)k->B2->d_live);
  if (source == LIVE_B2) {
    k->deadB = k->B2->n_inf;
    if (live_b_kept(source, k->deadB, nw, g16_env())) {
      HIPCHK(ctx, dev_alloc(k->liveB, bitmap_bytes));
      HIPCHK(ctx, hipMemcpyAsync(k->liveB.get(), k->B2->d_live.get(), bitmap_bytes, hipMemcpyDeviceToDevice, ctx->stream));
      HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    }
  } else if (source == LIVE_UNION) {
    uint32_t dead = 0;
    HIPCHK(ctx, dev_alloc(k->liveB, bitmap_bytes));
    const int32_t rc = counted_launch(ctx, 0, &dead, 1, [&](uint32_t* d_dead) {
      return g16_bitmap_or_device(ctx, k->liveB.get(), k->B1->d_live.get(), k->B2->d_live.get(), nw, d_dead);
    });
    if (rc) return rc;
    k->deadB = dead;
    if (!live_b_kept(source, dead, nw, g16_env())) k->liveB.reset();   // dense: share the witness sort
  }
  return G16_OK;
}

// 5. the A and B entries in row order, rows binned by length (sum order is irrelevant mod r)
static int32_t bin_coefficients(g16_ctx* ctx, const g16_pkey_desc* d, const CoeffSource& cs, g16_pkey* k) {
  const size_t n = size_t(1) << d->log2_domain;
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
  return g16_spmat_create(ctx, 2, (uint32_t)n, cs.count, vrow.data(), 4, (const uint32_t*)(cs.count ? cs.base + 8 : nullptr),
                          cs.stride, cs.count ? cs.base + cs.value_off : nullptr, cs.stride, &k->abc, cs.values_r2);
}

// table_stride: the stride of all five point sets (g16_points_register_*_lean; 0 / 1: a table per window)
static int32_t pkey_create(g16_ctx* ctx, const g16_pkey_desc* d, const CoeffSource& cs, uint32_t table_stride,
                           g16_pkey** out) {
  if (!desc_well_formed(d)) {
    ctx->err = "bad proving-key description";
    return G16_EINVAL;
  }
  CTX_ENTER(ctx);
  Building<g16_pkey, g16_pkey_destroy> k(new (std::nothrow) g16_pkey());
  if (!k) return G16_ENOMEM;
  const uint32_t ts = table_stride;
  int32_t rc;
  if ((rc = key_layout(ctx, d, k.get()))) return rc;
  const std::vector<unsigned char> c1pad = c1_wire_aligned(d, k.get());
  if ((rc = g16_points_register_g1_lean(ctx, (const char*)d->pointsA1 + 64 * k->w.lo, k->w.size(), ts, &k->A1))) return rc;
  if ((rc = b1_form_of_whole_arrays(ctx, d, k.get()))) return rc;
  if ((rc = register_b1(ctx, d, ts, k.get()))) return rc;
  if ((rc = g16_points_register_g2_lean(ctx, (const char*)d->pointsB2 + 128 * k->w.lo, k->w.size(), ts, &k->B2))) return rc;
  if ((rc = g16_points_register_g1_lean(ctx, c1pad.data(), k->w.size(), ts, &k->C1))) return rc;
  if ((rc = g16_points_register_g1_lean(ctx, (const char*)d->pointsH1 + 64 * k->h.lo, k->h.size(), ts, &k->H1))) return rc;
  if ((rc = live_lists(ctx, k.get()))) return rc;
  if ((rc = bin_coefficients(ctx, d, cs, k.get()))) return rc;
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
