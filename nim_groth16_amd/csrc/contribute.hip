// Phase-2 contribution (include/g16hip.h, "phase-2 contribution"): g16_key_contribute rescales the part of a key that
// holds delta, g16_contributions_verify walks a chain of contribution records from an initial key to a final one.  Host
// layer only, in the shape of a checker (checker.hpp): the scalings are scale_uniform (scale.cuh), the element checks
// audit.hip, the sums the one-shot MSM, the pairing equations the four-pair product of the circuit audit
// (circuit_audit.cuh).  Nothing is hashed or drawn here.
#include "checker.hpp"
#include "scale_plan.hpp"

using namespace g16;

namespace {

int32_t key_contribute(g16_ctx* ctx, const g16_phase2_key* key, const u256& d_mont, const u256& s_mont,
                       const void* challenge, g16_phase2_out* out) {
  int32_t rc;
  // 1. the element passes
  {
    const g16_audit_section sec[5] = {
        {1, key->delta1, 1}, {2, key->delta2, 1}, {1, key->pointsC1, key->nc1}, {1, key->pointsH1, key->nh1}, {2, challenge, 1}};
    ElementPass pass;
    if ((rc = pass.run(ctx, KEY_CONTRIBUTE_ARRAYS, sec)) || (rc = pass.first_finding(ctx, "g16_key_contribute"))) return rc;
  }

  // 2. the four scalars, standard form: d^-1 for the arrays, d, s and d s for the single points
  const u256 k_std[4] = {Fr::from_mont(Fr::inv(d_mont)), Fr::from_mont(d_mont), Fr::from_mont(s_mont),
                         Fr::from_mont(Fr::mul(d_mont, s_mont))};
  enum { K_DINV = 0, K_D, K_S, K_DS };
  ScalePlan plan[4];   // the host copies the uploads read: they live until the wait below
  ScaleJob job[4];
  const g1_aff gen1 = host_gen1();
  g1_aff small1[3];    // delta1 | gen1 | gen1 -> d delta1 | s gen1 | d s gen1
  g2_aff small2[2];    // delta2 | challenge   -> d delta2 | d challenge
  memcpy(&small1[0], key->delta1, sizeof(g1_aff));
  small1[1] = small1[2] = gen1;
  memcpy(&small2[0], key->delta2, sizeof(g2_aff));
  memcpy(&small2[1], challenge, sizeof(g2_aff));

  DevMem<g1_aff> d_c1, d_h1, d_small1;
  DevMem<g2_aff> d_small2;
  DevMem<uint32_t> d_steps;
  SyncOnExit drain{ctx->stream};
  auto up = [&](void* dst, const void* src, size_t bytes) {
    return bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, ctx->stream) : hipSuccess;
  };
  auto down = [&](void* dst, const void* src, size_t bytes) {
    return bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream) : hipSuccess;
  };
  HIPCHK(ctx, dev_alloc(d_c1, (key->nc1 ? key->nc1 : 1) * sizeof(g1_aff)));
  HIPCHK(ctx, dev_alloc(d_h1, (key->nh1 ? key->nh1 : 1) * sizeof(g1_aff)));
  HIPCHK(ctx, dev_alloc(d_small1, sizeof small1));
  HIPCHK(ctx, dev_alloc(d_small2, sizeof small2));
  HIPCHK(ctx, dev_alloc(d_steps, 4 * ScalePlan::MAX_STEPS * sizeof(uint32_t)));
  HIPCHK(ctx, up(d_c1.get(), key->pointsC1, key->nc1 * sizeof(g1_aff)));
  HIPCHK(ctx, up(d_h1.get(), key->pointsH1, key->nh1 * sizeof(g1_aff)));
  HIPCHK(ctx, up(d_small1.get(), small1, sizeof small1));
  HIPCHK(ctx, up(d_small2.get(), small2, sizeof small2));
  for (int k = 0; k < 4; ++k)
    if ((rc = g16_scale_job(ctx, k_std[k], plan[k], d_steps.get() + k * ScalePlan::MAX_STEPS, job[k]))) return rc;

  // 3. the scalings, in place
  if ((rc = scale_uniform_device<G1>(ctx, d_c1.get(), key->nc1, job[K_DINV], d_c1.get()))) return rc;
  if ((rc = scale_uniform_device<G1>(ctx, d_h1.get(), key->nh1, job[K_DINV], d_h1.get()))) return rc;
  if ((rc = scale_uniform_device<G1>(ctx, d_small1.get(), 1, job[K_D], d_small1.get()))) return rc;
  if ((rc = scale_uniform_device<G1>(ctx, d_small1.get() + 1, 1, job[K_S], d_small1.get() + 1))) return rc;
  if ((rc = scale_uniform_device<G1>(ctx, d_small1.get() + 2, 1, job[K_DS], d_small1.get() + 2))) return rc;
  if ((rc = scale_uniform_device<G2>(ctx, d_small2.get(), 2, job[K_D], d_small2.get()))) return rc;

  // 4. to the caller
  HIPCHK(ctx, down(out->pointsC1, d_c1.get(), key->nc1 * sizeof(g1_aff)));
  HIPCHK(ctx, down(out->pointsH1, d_h1.get(), key->nh1 * sizeof(g1_aff)));
  HIPCHK(ctx, down(small1, d_small1.get(), sizeof small1));
  HIPCHK(ctx, down(small2, d_small2.get(), sizeof small2));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  memcpy(out->delta1, &small1[0], sizeof(g1_aff));
  memcpy(out->delta2, &small2[0], sizeof(g2_aff));
  memcpy(out->record->delta_after, &small1[0], 64);
  memcpy(out->record->g1_s, &small1[1], 64);
  memcpy(out->record->g1_sx, &small1[2], 64);
  memcpy(out->record->g2_spx, &small2[1], 128);
  return G16_OK;
}

int32_t contributions_verify(g16_ctx* ctx, const g16_phase2_key* ini, const g16_phase2_key* fin,
                             const g16_contribution* rec, const void* challenges, size_t count,
                             const std::vector<uint64_t>& z, const std::vector<uint64_t>& y, g16_chain_report* out) {
  int32_t rc;
  const size_t nc1 = ini->nc1, nh1 = ini->nh1;
  // 1. ELEMENTS: the record fields as arrays of their own, then the passes and the scan for (0,0)
  std::vector<g1_aff> after(count), gs(count), gsx(count);
  std::vector<g2_aff> spx(count);
  for (size_t j = 0; j < count; ++j) {
    memcpy(&after[j], rec[j].delta_after, 64);
    memcpy(&gs[j], rec[j].g1_s, 64);
    memcpy(&gsx[j], rec[j].g1_sx, 64);
    memcpy(&spx[j], rec[j].g2_spx, 128);
  }
  const g16_audit_section sec[G16_CHAIN_ARRAYS] = {
      {1, after.data(), count}, {1, gs.data(), count},  {1, gsx.data(), count},     {2, spx.data(), count},
      {2, challenges, count},   {1, fin->delta1, 1},    {2, fin->delta2, 1},        {1, fin->pointsC1, nc1},
      {1, fin->pointsH1, nh1}};
  ElementPass pass;
  if ((rc = pass.run(ctx, CHAIN_ARRAYS, sec))) return rc;
  pass.to_report(out->first_bad, out->bad_count, out->first_infinity);
  bool run[G16_CHAIN_RELATIONS];
  relations_run(CHAIN_RELATIONS, pass.clean(), 0, run);

  // 2. the products, each e(P0, Q0) e(-P1, Q1): POK_j at 2j, STEP_j at 2j + 1, then DELTA, C1, H1
  const size_t i_delta = 2 * count, i_c1 = i_delta + 1, i_h1 = i_delta + 2;
  ProductTable pt(2 * count + 3);
  SyncOnExit drain{ctx->stream};
  const g1_aff gen1 = host_gen1();
  const g2_aff gen2 = host_gen2();
  const g2_aff* sp = (const g2_aff*)challenges;
  for (size_t j = 0; j < count; ++j) {
    if (run[G16_CHAIN_POK]) pt.set(2 * j, 0, &gs[j], &spx[j]), pt.set(2 * j, 1, &gsx[j], &sp[j]);
    if (run[G16_CHAIN_STEP])
      pt.set(2 * j + 1, 0, j ? (const void*)&after[j - 1] : ini->delta1, &spx[j]), pt.set(2 * j + 1, 1, &after[j], &sp[j]);
  }
  if (run[G16_CHAIN_DELTA]) pt.set(i_delta, 0, fin->delta1, &gen2), pt.set(i_delta, 1, &gen1, fin->delta2);
  for (size_t i : {i_c1, i_h1}) pt.set(i, 0, nullptr, ini->delta2), pt.set(i, 1, nullptr, fin->delta2);
  if ((rc = pt.upload(ctx))) return rc;
  // 3. the four sums, straight into their slots: each multiplier vector is uploaded once
  if (run[G16_CHAIN_C1]) {
    if ((rc = stage_scalars(ctx, z.data(), nc1))) return rc;
    if ((rc = staged_msm<G1>(ctx, ctx->stage_s.p(), G16_SCALARS_STD, ini->pointsC1, nc1, pt.d_P(i_c1, 0)))) return rc;
    if ((rc = staged_msm<G1>(ctx, ctx->stage_s.p(), G16_SCALARS_STD, fin->pointsC1, nc1, pt.d_P(i_c1, 1)))) return rc;
  }
  if (run[G16_CHAIN_H1]) {
    if ((rc = stage_scalars(ctx, y.data(), nh1))) return rc;
    if ((rc = staged_msm<G1>(ctx, ctx->stage_s.p(), G16_SCALARS_STD, ini->pointsH1, nh1, pt.d_P(i_h1, 0)))) return rc;
    if ((rc = staged_msm<G1>(ctx, ctx->stage_s.p(), G16_SCALARS_STD, fin->pointsH1, nh1, pt.d_P(i_h1, 1)))) return rc;
  }
  // 4. every product in one launch
  if ((rc = pt.run(ctx, 2u))) return rc;
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));

  // 5. the verdicts
  int32_t* rel = out->relation;
  rel[G16_CHAIN_ELEMENTS] = pass.all_clean() ? 1 : 0;
  if (run[G16_CHAIN_LAST])
    rel[G16_CHAIN_LAST] = !memcmp(fin->delta1, count ? (const void*)rec[count - 1].delta_after : ini->delta1, 64);
  if (run[G16_CHAIN_DELTA]) rel[G16_CHAIN_DELTA] = pt.result(i_delta);
  if (run[G16_CHAIN_C1]) rel[G16_CHAIN_C1] = pt.result(i_c1);
  if (run[G16_CHAIN_H1]) rel[G16_CHAIN_H1] = pt.result(i_h1);
  fold_report(CHAIN_RELATIONS, run, pt.res.data(), count, rel, out->first_record, out->failed);
  return G16_OK;
}

}  // namespace

extern "C" int32_t g16_key_contribute(g16_ctx* ctx, const g16_phase2_key* key, const void* d, const void* s,
                                      uint32_t flags, const void* challenge_g2, g16_phase2_out* out) {
  if (!ctx) return G16_EINVAL;
  static const char who[] = "g16_key_contribute";
  if (!key || !d || !s || !challenge_g2 || !out) return fail(ctx, who, "null argument");
  if (!key->delta1 || !key->delta2 || (key->nc1 && !key->pointsC1) || (key->nh1 && !key->pointsH1))
    return fail(ctx, who, "null key pointer");
  if (!out->delta1 || !out->delta2 || (key->nc1 && !out->pointsC1) || (key->nh1 && !out->pointsH1) || !out->record)
    return fail(ctx, who, "null output pointer");
  if (flags != G16_SCALARS_MONT && flags != G16_SCALARS_STD)
    return fail(ctx, who, "flags must be G16_SCALARS_MONT or G16_SCALARS_STD");
  if (key->nc1 >= (size_t(1) << 31) || key->nh1 >= (size_t(1) << 31))
    return fail(ctx, who, "array too long (must be < 2^31 points)");
  u256 d_mont, s_mont;
  if (!load_scalar_nonzero_mont(d, flags == G16_SCALARS_MONT, d_mont))
    return fail(ctx, who, "d must be non-zero and canonical (< r)");
  if (!load_scalar_nonzero_mont(s, flags == G16_SCALARS_MONT, s_mont))
    return fail(ctx, who, "s must be non-zero and canonical (< r)");
  if (is_infinity(key->delta1, 64)) return fail(ctx, who, "delta1 is the point at infinity");
  if (is_infinity(key->delta2, 128)) return fail(ctx, who, "delta2 is the point at infinity");
  if (is_infinity(challenge_g2, 128)) return fail(ctx, who, "the challenge is the point at infinity");
  CTX_ENTER(ctx);
  return key_contribute(ctx, key, d_mont, s_mont, challenge_g2, out);
}

extern "C" int32_t g16_contributions_verify(g16_ctx* ctx, const g16_phase2_key* initial, const g16_phase2_key* final_,
                                            const g16_contribution* records, const void* challenges_g2, size_t count,
                                            const void* c1_multipliers, const void* h1_multipliers,
                                            g16_chain_report* out) {
  if (!ctx) return G16_EINVAL;
  static const char who[] = "g16_contributions_verify";
  if (!initial || !final_ || !out || (count && (!records || !challenges_g2))) return fail(ctx, who, "null argument");
  if (initial->nc1 != final_->nc1 || initial->nh1 != final_->nh1)
    return fail(ctx, who, "the initial and the final key have other point counts (nc1, nh1)");
  for (const g16_phase2_key* k : {initial, final_})
    if (!k->delta1 || !k->delta2 || (k->nc1 && !k->pointsC1) || (k->nh1 && !k->pointsH1))
      return fail(ctx, who, "null key pointer");
  if ((initial->nc1 && !c1_multipliers) || (initial->nh1 && !h1_multipliers)) return fail(ctx, who, "null multipliers");
  if (count >= (size_t(1) << 20)) return fail(ctx, who, "too many records (count must be < 2^20)");
  if (initial->nc1 >= (size_t(1) << 27) || initial->nh1 >= (size_t(1) << 27))
    return fail(ctx, who, "array too long (must be < 2^27 points)");
  return no_throw(ctx, [&]() -> int32_t {   // the record arrays and the widened multipliers live in host vectors
    std::vector<uint64_t> z, y;
    int32_t rc;
    if ((rc = g16_widen_multipliers(ctx, "g16_contributions_verify: c1", c1_multipliers, initial->nc1, z))) return rc;
    if ((rc = g16_widen_multipliers(ctx, "g16_contributions_verify: h1", h1_multipliers, initial->nh1, y))) return rc;
    report_reset(out);
    CTX_ENTER(ctx);
    return contributions_verify(ctx, initial, final_, records, challenges_g2, count, z, y, out);
  });
}
