// Phase-1 contribution (include/g16hip.h, "phase-1 contribution"): g16_ptau_contribute takes the powers of (tau, alpha,
// beta) to those of (t tau, a alpha, b beta); g16_ptau_verify checks such powers and a chain of records with the one-shot
// MSM and the four-pair product of the circuit audit.  Host layer only, in the shape of a checker (checker.hpp): the scalars
// c t^i are the geometric-sequence kernel of the setup (setup.hip), the scalings scale_each (scale_each.cuh), the element
// checks audit.hip.  Nothing is hashed or drawn.
#include <cstdlib>

#include "checker.hpp"

using namespace g16;

namespace {

constexpr uint32_t PTAU_MAX_POWER = 25;
constexpr size_t PTAU_CHUNK = size_t(1) << 22;   // points of a long array on the device at a time

// the chunk of this call: PTAU_CHUNK, or fewer points if G16_PTAU_CHUNK says so (the tests walk the chunk loop at power 3)
size_t ptau_chunk() {
  const char* e = getenv("G16_PTAU_CHUNK");
  const unsigned long long v = e ? strtoull(e, nullptr, 10) : 0;
  return v && v < PTAU_CHUNK ? (size_t)v : PTAU_CHUNK;
}

u256 fr_pow(u256 x, uint64_t e) {
  u256 acc = Fr::one();
  for (; e; e >>= 1, x = Fr::sqr(x))
    if (e & 1) acc = Fr::mul(acc, x);
  return acc;
}

struct Scratch {
  DevMem<> pts;       // PTAU_CHUNK G2 points (or as many as the longest array has)
  DevMem<u256> k;     // as many scalars
};

// out[i] = c t^i * in[i], i < n: chunk by chunk through `s`, every step in stream order
template <class C>
int32_t scale_array(g16_ctx* ctx, Scratch& s, size_t chunk, const void* in, size_t n, const u256& t_mont, const u256& c_std,
                    void* out) {
  constexpr size_t psz = sizeof(typename C::Aff);
  for (size_t at = 0; at < n; at += chunk) {
    const size_t m = n - at < chunk ? n - at : chunk;
    int32_t rc;
    HIPCHK(ctx, hipMemcpyAsync(s.pts.get(), (const char*)in + at * psz, m * psz, hipMemcpyHostToDevice, ctx->stream));
    // Montgomery t^at t^i times the integer c: the standard form of c t^(at + i)
    if ((rc = g16_setup_geometric(ctx, false, fr_pow(t_mont, at), t_mont, c_std, Fr::zero(), m, s.k.get(), nullptr)))
      return rc;
    if ((rc = scale_each_device<C>(ctx, s.pts.get(), m, s.k.get(), 0u, s.pts.get()))) return rc;
    HIPCHK(ctx, hipMemcpyAsync((char*)out + at * psz, s.pts.get(), m * psz, hipMemcpyDeviceToHost, ctx->stream));
  }
  return G16_OK;
}

int32_t ptau_contribute(g16_ctx* ctx, const g16_ptau_desc* ptau, const u256 (&x)[3], const u256 (&sx)[3],
                        const void* challenges, g16_ptau_out* out, g16_ptau_contribution* record) {
  const size_t n = size_t(1) << ptau->power, n1 = 2 * n - 1;
  int32_t rc;
  // 1. the element passes, then the scan for (0,0)
  {
    const g16_audit_section sec[6] = {{1, ptau->tauG1, n1},    {2, ptau->tauG2, n}, {1, ptau->alphaTauG1, n},
                                      {1, ptau->betaTauG1, n}, {2, ptau->betaG2, 1}, {2, challenges, 3}};
    ElementPass pass;
    if ((rc = pass.run(ctx, PTAU_CONTRIBUTE_ARRAYS, sec)) || (rc = pass.first_finding(ctx, "g16_ptau_contribute"))) return rc;
  }

  // 2. the single points: s gen1 and x s gen1 for x = t, a, b; b betaG2 and x challenge_x
  const u256 one_std = Fr::from_mont(Fr::one());
  const g1_aff gen1 = host_gen1();
  g1_aff small1[6];
  g2_aff small2[4];
  u256 k1[6], k2[4];   // Montgomery form; the host copies the uploads read: they live until the wait below
  for (int j = 0; j < 3; ++j) {
    small1[2 * j] = small1[2 * j + 1] = gen1;
    k1[2 * j] = sx[j], k1[2 * j + 1] = Fr::mul(x[j], sx[j]);
    memcpy(&small2[1 + j], (const char*)challenges + sizeof(g2_aff) * j, sizeof(g2_aff));
    k2[1 + j] = x[j];
  }
  memcpy(&small2[0], ptau->betaG2, sizeof(g2_aff));
  k2[0] = x[2];

  Scratch s;
  DevMem<g1_aff> d_small1;
  DevMem<g2_aff> d_small2;
  DevMem<u256> d_k1, d_k2;
  SyncOnExit drain{ctx->stream};
  const size_t chunk = n1 < ptau_chunk() ? n1 : ptau_chunk();
  HIPCHK(ctx, dev_alloc(s.pts, chunk * sizeof(g2_aff)));
  HIPCHK(ctx, dev_alloc(s.k, chunk * sizeof(u256)));
  HIPCHK(ctx, dev_alloc(d_small1, sizeof small1));
  HIPCHK(ctx, dev_alloc(d_small2, sizeof small2));
  HIPCHK(ctx, dev_alloc(d_k1, sizeof k1));
  HIPCHK(ctx, dev_alloc(d_k2, sizeof k2));
  HIPCHK(ctx, hipMemcpyAsync(d_small1.get(), small1, sizeof small1, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(d_small2.get(), small2, sizeof small2, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(d_k1.get(), k1, sizeof k1, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(d_k2.get(), k2, sizeof k2, hipMemcpyHostToDevice, ctx->stream));
  if ((rc = scale_each_device<G1>(ctx, d_small1.get(), 6, d_k1.get(), 1u, d_small1.get()))) return rc;
  if ((rc = scale_each_device<G2>(ctx, d_small2.get(), 4, d_k2.get(), 1u, d_small2.get()))) return rc;

  // 3. the four arrays
  const u256 a_std = Fr::from_mont(x[1]), b_std = Fr::from_mont(x[2]);
  if ((rc = scale_array<G1>(ctx, s, chunk, ptau->tauG1, n1, x[0], one_std, out->tauG1))) return rc;
  if ((rc = scale_array<G2>(ctx, s, chunk, ptau->tauG2, n, x[0], one_std, out->tauG2))) return rc;
  if ((rc = scale_array<G1>(ctx, s, chunk, ptau->alphaTauG1, n, x[0], a_std, out->alphaTauG1))) return rc;
  if ((rc = scale_array<G1>(ctx, s, chunk, ptau->betaTauG1, n, x[0], b_std, out->betaTauG1))) return rc;

  // 4. to the caller
  HIPCHK(ctx, hipMemcpyAsync(small1, d_small1.get(), sizeof small1, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(small2, d_small2.get(), sizeof small2, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  memcpy(out->betaG2, &small2[0], sizeof(g2_aff));
  memcpy(record->tauG1, (const char*)out->tauG1 + sizeof(g1_aff), sizeof(g1_aff));
  memcpy(record->alphaG1, out->alphaTauG1, sizeof(g1_aff));
  memcpy(record->betaG1, out->betaTauG1, sizeof(g1_aff));
  memcpy(record->tauG2, (const char*)out->tauG2 + sizeof(g2_aff), sizeof(g2_aff));
  memcpy(record->betaG2, &small2[0], sizeof(g2_aff));
  for (int j = 0; j < 3; ++j) {
    memcpy(record->pok[j].g1_s, &small1[2 * j], sizeof(g1_aff));
    memcpy(record->pok[j].g1_sx, &small1[2 * j + 1], sizeof(g1_aff));
    memcpy(record->pok[j].g2_spx, &small2[1 + j], sizeof(g2_aff));
  }
  return G16_OK;
}

// ---- g16_ptau_verify ------------------------------------------------------------------------------------------------------
int32_t ptau_verify(g16_ctx* ctx, const g16_ptau_desc* ptau, const g16_ptau_contribution* rec, const void* challenges,
                    size_t count, bool chain, const std::vector<uint64_t>& z, g16_ptau_report* out) {
  int32_t rc;
  const size_t n = size_t(1) << ptau->power, n1 = 2 * n - 1;
  const g1_aff gen1 = host_gen1();
  const g2_aff gen2 = host_gen2();
  // 1. ELEMENTS: the record fields as arrays of their own, then the passes and the scan for (0,0)
  std::vector<g1_aff> r1[3], gs(3 * count), gsx(3 * count);   // r1: tauG1, alphaG1, betaG1 after each record
  std::vector<g2_aff> r2[2], spx(3 * count);                  // r2: tauG2, betaG2
  for (auto& v : r1) v.resize(count);
  for (auto& v : r2) v.resize(count);
  for (size_t j = 0; j < count; ++j) {
    memcpy(&r1[0][j], rec[j].tauG1, 64), memcpy(&r1[1][j], rec[j].alphaG1, 64), memcpy(&r1[2][j], rec[j].betaG1, 64);
    memcpy(&r2[0][j], rec[j].tauG2, 128), memcpy(&r2[1][j], rec[j].betaG2, 128);
    for (int x = 0; x < 3; ++x) {
      memcpy(&gs[3 * j + x], rec[j].pok[x].g1_s, 64), memcpy(&gsx[3 * j + x], rec[j].pok[x].g1_sx, 64);
      memcpy(&spx[3 * j + x], rec[j].pok[x].g2_spx, 128);
    }
  }
  const g16_audit_section sec[G16_PTAU_REPORT_ARRAYS] = {
      {1, ptau->tauG1, n1},       {2, ptau->tauG2, n},        {1, ptau->alphaTauG1, n},   {1, ptau->betaTauG1, n},
      {2, ptau->betaG2, 1},       {1, r1[0].data(), count},   {1, r1[1].data(), count},   {1, r1[2].data(), count},
      {2, r2[0].data(), count},   {2, r2[1].data(), count},   {1, gs.data(), 3 * count},  {1, gsx.data(), 3 * count},
      {2, spx.data(), 3 * count}, {2, challenges, 3 * count}};
  ElementPass pass;
  if ((rc = pass.run(ctx, PTAU_ARRAYS, sec))) return rc;
  pass.to_report(out->first_bad, out->bad_count, out->first_infinity);
  bool run[G16_PTAU_RELATIONS];
  relations_run(PTAU_RELATIONS, pass.clean(), chain ? NEED_RECORDS : 0, run);

  // 2. the products, each e(P0, Q0) e(-P1, Q1): TAU_G1, TAU_G2, ALPHA, BETA, BETA_G2, then per record three POK and five STEP
  enum { I_TAU1 = 0, I_TAU2, I_ALPHA, I_BETA, I_BG2, FIXED = PTAU_FIXED_ROWS };
  ProductTable pt(FIXED + 8 * count);
  SyncOnExit drain{ctx->stream};
  const g1_aff* tau1 = (const g1_aff*)ptau->tauG1;
  const g2_aff* tau2 = (const g2_aff*)ptau->tauG2;
  const g2_aff* ch = (const g2_aff*)challenges;
  if (run[G16_PTAUV_TAU_G1]) {   // and FIRST, TAU_G2: the same arrays
    pt.set(I_TAU1, 0, nullptr, tau2 + 1), pt.set(I_TAU1, 1, nullptr, &gen2);
    pt.set(I_TAU2, 0, tau1 + 1, nullptr), pt.set(I_TAU2, 1, &gen1, nullptr);
  }
  if (run[G16_PTAUV_ALPHA]) pt.set(I_ALPHA, 0, nullptr, tau2 + 1), pt.set(I_ALPHA, 1, nullptr, &gen2);
  if (run[G16_PTAUV_BETA]) pt.set(I_BETA, 0, nullptr, tau2 + 1), pt.set(I_BETA, 1, nullptr, &gen2);
  if (run[G16_PTAUV_BETA_G2]) pt.set(I_BG2, 0, ptau->betaTauG1, &gen2), pt.set(I_BG2, 1, &gen1, ptau->betaG2);
  for (size_t j = 0; j < count; ++j) {
    const size_t base = FIXED + 8 * j;
    for (int x = 0; x < 3; ++x) {
      const size_t k = 3 * j + x;
      if (run[G16_PTAUV_POK]) pt.set(base + x, 0, &gs[k], &spx[k]), pt.set(base + x, 1, &gsx[k], ch + k);
      if (run[G16_PTAUV_STEP])   // the G1 value that x moves: tauG1 by t, alphaG1 by a, betaG1 by b
        pt.set(base + 3 + x, 0, j ? &r1[x][j - 1] : &gen1, &spx[k]), pt.set(base + 3 + x, 1, &r1[x][j], ch + k);
    }
    if (run[G16_PTAUV_STEP])
      for (int y = 0; y < 2; ++y) {   // tauG2 moves by t (pok 0), betaG2 by b (pok 2)
        const size_t k = 3 * j + (y ? 2 : 0);
        pt.set(base + 6 + y, 0, &gsx[k], j ? &r2[y][j - 1] : &gen2), pt.set(base + 6 + y, 1, &gs[k], &r2[y][j]);
      }
  }
  if ((rc = pt.upload(ctx))) return rc;
  // 3. the sums: the multipliers once, every array uploaded once and summed at the point offsets 0 and 1
  if ((rc = stage_scalars(ctx, z.data(), n1 - 1))) return rc;
  const void* d_z = ctx->stage_s.p();
  if (run[G16_PTAUV_TAU_G1]) {
    if ((rc = staged_msm<G1>(ctx, d_z, G16_SCALARS_STD, ptau->tauG1, n1 - 1, pt.d_P(I_TAU1, 0), 2))) return rc;
    if ((rc = staged_msm<G2>(ctx, d_z, G16_SCALARS_STD, ptau->tauG2, n - 1, pt.d_Q(I_TAU2, 0), 2))) return rc;
  }
  if (run[G16_PTAUV_ALPHA] && (rc = staged_msm<G1>(ctx, d_z, G16_SCALARS_STD, ptau->alphaTauG1, n - 1, pt.d_P(I_ALPHA, 0), 2)))
    return rc;
  if (run[G16_PTAUV_BETA] && (rc = staged_msm<G1>(ctx, d_z, G16_SCALARS_STD, ptau->betaTauG1, n - 1, pt.d_P(I_BETA, 0), 2)))
    return rc;
  // 4. every product in one launch
  if ((rc = pt.run(ctx, 2u))) return rc;
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));

  // 5. the verdicts
  int32_t* rel = out->relation;
  rel[G16_PTAUV_ELEMENTS] = pass.all_clean() ? 1 : 0;
  if (run[G16_PTAUV_FIRST]) {
    rel[G16_PTAUV_FIRST] = !memcmp(ptau->tauG1, &gen1, 64) && !memcmp(ptau->tauG2, &gen2, 128);
    rel[G16_PTAUV_TAU_G1] = pt.result(I_TAU1), rel[G16_PTAUV_TAU_G2] = pt.result(I_TAU2);
  }
  if (run[G16_PTAUV_ALPHA]) rel[G16_PTAUV_ALPHA] = pt.result(I_ALPHA);
  if (run[G16_PTAUV_BETA]) rel[G16_PTAUV_BETA] = pt.result(I_BETA);
  if (run[G16_PTAUV_BETA_G2]) rel[G16_PTAUV_BETA_G2] = pt.result(I_BG2);
  if (run[G16_PTAUV_LAST]) {
    const void* last[5] = {count ? (const void*)rec[count - 1].tauG1 : &gen1, count ? (const void*)rec[count - 1].alphaG1 : &gen1,
                           count ? (const void*)rec[count - 1].betaG1 : &gen1, count ? (const void*)rec[count - 1].tauG2 : &gen2,
                           count ? (const void*)rec[count - 1].betaG2 : &gen2};
    rel[G16_PTAUV_LAST] = !memcmp((const char*)ptau->tauG1 + 64, last[0], 64) && !memcmp(ptau->alphaTauG1, last[1], 64) &&
                          !memcmp(ptau->betaTauG1, last[2], 64) && !memcmp((const char*)ptau->tauG2 + 128, last[3], 128) &&
                          !memcmp(ptau->betaG2, last[4], 128);
  }
  fold_report(PTAU_RELATIONS, run, pt.res.data() + FIXED, count, rel, out->first_record, out->failed);
  return G16_OK;
}

}  // namespace

static_assert(sizeof(g16_ptau_contribution) == 1216, "a phase-1 record is 1216 bytes");

extern "C" int32_t g16_ptau_contribute(g16_ctx* ctx, const g16_ptau_desc* ptau, const void* t, const void* a, const void* b,
                                       const void* s3, uint32_t flags, const void* challenges_g2, g16_ptau_out* out,
                                       g16_ptau_contribution* record) {
  if (!ctx) return G16_EINVAL;
  static const char who[] = "g16_ptau_contribute";
  if (!ptau || !t || !a || !b || !s3 || !challenges_g2 || !out || !record) return fail(ctx, who, "null argument");
  if (!ptau->tauG1 || !ptau->tauG2 || !ptau->alphaTauG1 || !ptau->betaTauG1 || !ptau->betaG2)
    return fail(ctx, who, "null ptau pointer");
  if (!out->tauG1 || !out->tauG2 || !out->alphaTauG1 || !out->betaTauG1 || !out->betaG2)
    return fail(ctx, who, "null output pointer");
  if (flags != G16_SCALARS_MONT && flags != G16_SCALARS_STD)
    return fail(ctx, who, "flags must be G16_SCALARS_MONT or G16_SCALARS_STD");
  if (ptau->power == 0 || ptau->power > PTAU_MAX_POWER) return fail(ctx, who, "power out of range (must be 1..25)");
  const bool mont = flags == G16_SCALARS_MONT;
  u256 x[3], sx[3];
  if (!load_scalar_nonzero_mont(t, mont, x[0])) return fail(ctx, who, "t must be non-zero and canonical (< r)");
  if (!load_scalar_nonzero_mont(a, mont, x[1])) return fail(ctx, who, "a must be non-zero and canonical (< r)");
  if (!load_scalar_nonzero_mont(b, mont, x[2])) return fail(ctx, who, "b must be non-zero and canonical (< r)");
  for (int j = 0; j < 3; ++j)
    if (!load_scalar_nonzero_mont((const char*)s3 + 32 * j, mont, sx[j]))
      return fail(ctx, who, "s must be non-zero and canonical (< r), all three");
  CTX_ENTER(ctx);
  return no_throw(ctx, [&] { return ptau_contribute(ctx, ptau, x, sx, challenges_g2, out, record); });   // the error texts
}

extern "C" int32_t g16_ptau_verify(g16_ctx* ctx, const g16_ptau_desc* ptau, const g16_ptau_contribution* records,
                                   const void* challenges_g2, size_t count, const void* multipliers, g16_ptau_report* out) {
  if (!ctx) return G16_EINVAL;
  static const char who[] = "g16_ptau_verify";
  if (!ptau || !multipliers || !out || (count && (!records || !challenges_g2))) return fail(ctx, who, "null argument");
  if (!ptau->tauG1 || !ptau->tauG2 || !ptau->alphaTauG1 || !ptau->betaTauG1 || !ptau->betaG2)
    return fail(ctx, who, "null ptau pointer");
  if (ptau->power == 0 || ptau->power > PTAU_MAX_POWER) return fail(ctx, who, "power out of range (must be 1..25)");
  if (count >= (size_t(1) << 16)) return fail(ctx, who, "too many records (count must be < 2^16)");
  return no_throw(ctx, [&]() -> int32_t {   // the record arrays and the widened multipliers live in host vectors
    std::vector<uint64_t> z;
    if (int32_t rc = g16_widen_multipliers(ctx, who, multipliers, (size_t(2) << ptau->power) - 2, z)) return rc;
    report_reset(out);
    CTX_ENTER(ctx);
    return ptau_verify(ctx, ptau, records, challenges_g2, count, records != nullptr, z, out);
  });
}
