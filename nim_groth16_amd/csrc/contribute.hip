// Phase-2 contribution (include/g16hip.h, "phase-2 contribution"): g16_key_contribute rescales the part of a key that
// holds delta, g16_contributions_verify walks a chain of contribution records from an initial key to a final one.  Host
// layer only: the scalings are scale_uniform (scale.cuh), the element checks audit.hip, the sums the one-shot MSM, the
// pairing equations the four-pair product of the circuit audit (circuit_audit.cuh).  Nothing is hashed or drawn here.
#include <new>

#include "g16_internal.hpp"
#include "ec.cuh"
#include "scale_plan.hpp"

using namespace g16;

void g16_curve_consts_g2(void* gen2, void* twist_b);   // msm_g2_misc.hip: gen2 (128 B), twistCoeffB (64 B)

namespace {

constexpr size_t NONE = (size_t)-1;
const char* const WHAT[3] = {"is not a canonical encoding", "is not on the curve", "is not in the order-r subgroup"};

bool all_zero(const void* p, size_t bytes) {
  const unsigned char* b = (const unsigned char*)p;
  for (size_t i = 0; i < bytes; ++i)
    if (b[i]) return false;
  return true;
}

// a 32-byte scalar of the caller, canonical and non-zero, to standard form
bool load_nonzero(const void* p, bool mont, u256& std_out) {
  u256 v;
  memcpy(&v, p, 32);
  if (!Fr::is_canonical(v) || Fr::is_zero(v)) return false;
  std_out = mont ? Fr::from_mont(v) : v;
  return true;
}

int32_t key_contribute(g16_ctx* ctx, const g16_phase2_key* key, const u256& d_std, const u256& s_std,
                       const void* challenge, g16_phase2_out* out) {
  auto bad = [&](const std::string& msg) {
    ctx->err = "g16_key_contribute: " + msg;
    return G16_EINVAL;
  };
  int32_t rc;
  // 1. the element passes
  {
    enum { NSEC = 5 };
    static const char* const names[NSEC] = {"delta1", "delta2", "pointsC1", "pointsH1", "challenge"};
    const g16_audit_section sec[NSEC] = {
        {1, key->delta1, 1}, {2, key->delta2, 1}, {1, key->pointsC1, key->nc1}, {1, key->pointsH1, key->nh1}, {2, challenge, 1}};
    size_t first_bad[NSEC][3], bad_count[NSEC][3];
    if ((rc = g16_audit_sections(ctx, sec, NSEC, first_bad, bad_count))) return rc;
    for (int s = 0; s < NSEC; ++s)
      for (int k = 0; k < 3; ++k) {
        if (!bad_count[s][k]) continue;
        std::string text = std::string(names[s]) + "[" + std::to_string(first_bad[s][k]) + "] " + WHAT[k];
        if (bad_count[s][k] > 1) text += " (and " + std::to_string(bad_count[s][k] - 1) + " more)";
        return bad(text);
      }
  }

  // 2. the four scalars: d^-1 for the arrays, d, s and d s for the single points
  const u256 d_mont = Fr::to_mont(d_std), s_mont = Fr::to_mont(s_std);
  const u256 k_std[4] = {Fr::from_mont(Fr::inv(d_mont)), d_std, s_std, Fr::from_mont(Fr::mul(d_mont, s_mont))};
  enum { K_DINV = 0, K_D, K_S, K_DS };
  ScalePlan plan[4];   // the host copies the uploads read: they live until the wait below
  ScaleJob job[4];
  const g1_aff gen1{Fp::one(), Fp::dbl(Fp::one())};
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

// sum_i s_i P_i for a HOST point array (through the context's staging buffers) and HOST standard-form scalars
int32_t msm_host(g16_ctx* ctx, const uint64_t* scalars, const void* points, size_t n, void* d_out) {
  if (!n) return G16_OK;   // the slot keeps (0,0)
  int32_t rc;
  if ((rc = ensure(ctx, ctx->stage_s, n * 32))) return rc;
  if ((rc = ensure(ctx, ctx->stage_p, n * sizeof(g1_aff)))) return rc;
  HIPCHK(ctx, hipMemcpyAsync(ctx->stage_s.p(), scalars, n * 32, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(ctx->stage_p.p(), points, n * sizeof(g1_aff), hipMemcpyHostToDevice, ctx->stream));
  return msm_device<G1>(ctx, ctx->stage_s.p(), G16_SCALARS_STD, ctx->stage_p.p(), n, d_out, nullptr, 0);
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
  if ((rc = g16_audit_sections(ctx, sec, G16_CHAIN_ARRAYS, out->first_bad, out->bad_count))) return rc;
  bool clean[G16_CHAIN_ARRAYS];
  bool elements = true;
  for (int a = 0; a < G16_CHAIN_ARRAYS; ++a) {
    clean[a] = !(out->bad_count[a][0] | out->bad_count[a][1] | out->bad_count[a][2]);
    if (a <= G16_CHAIN_FINAL_DELTA2) {
      const size_t psz = sec[a].group == 1 ? sizeof(g1_aff) : sizeof(g2_aff);
      for (size_t j = 0; j < sec[a].n; ++j)
        if (all_zero((const char*)sec[a].p + psz * j, psz)) {
          out->first_infinity[a] = j;
          clean[a] = false;
          break;
        }
    }
    elements = elements && clean[a];
  }
  const bool run_pok = clean[G16_CHAIN_G1_S] && clean[G16_CHAIN_G1_SX] && clean[G16_CHAIN_G2_SPX] && clean[G16_CHAIN_CHALLENGES];
  const bool run_step = clean[G16_CHAIN_DELTA_AFTER] && clean[G16_CHAIN_G2_SPX] && clean[G16_CHAIN_CHALLENGES];
  const bool run_last = clean[G16_CHAIN_DELTA_AFTER] && clean[G16_CHAIN_FINAL_DELTA1];
  const bool run_delta = clean[G16_CHAIN_FINAL_DELTA1] && clean[G16_CHAIN_FINAL_DELTA2];
  const bool run_c1 = clean[G16_CHAIN_FINAL_DELTA2] && clean[G16_CHAIN_FINAL_POINTS_C1];
  const bool run_h1 = clean[G16_CHAIN_FINAL_DELTA2] && clean[G16_CHAIN_FINAL_POINTS_H1];

  // 2. the products: POK_j at 2j, STEP_j at 2j + 1, then DELTA, C1, H1.  Each is e(P0, Q0) e(-P1, Q1); pairs 2 and 3, and
  //    every product that is not run, keep (0,0) and contribute one.
  const size_t nprod = 2 * count + 3, i_delta = 2 * count, i_c1 = i_delta + 1, i_h1 = i_delta + 2;
  std::vector<g1_aff> P(4 * nprod);
  std::vector<g2_aff> Q(4 * nprod);
  std::vector<int32_t> result(nprod, 0);
  memset(P.data(), 0, P.size() * sizeof(g1_aff));
  memset(Q.data(), 0, Q.size() * sizeof(g2_aff));
  const g1_aff gen1{Fp::one(), Fp::dbl(Fp::one())};
  g2_aff gen2;
  {
    fp2_t twist_b;
    g16_curve_consts_g2(&gen2, &twist_b);
  }
  const g2_aff* sp = (const g2_aff*)challenges;
  for (size_t j = 0; j < count; ++j) {
    if (run_pok) {
      P[8 * j] = gs[j], Q[8 * j] = spx[j];
      P[8 * j + 1] = gsx[j], memcpy(&Q[8 * j + 1], &sp[j], sizeof(g2_aff));
    }
    if (run_step) {
      if (j) P[8 * j + 4] = after[j - 1];
      else memcpy(&P[8 * j + 4], ini->delta1, sizeof(g1_aff));
      Q[8 * j + 4] = spx[j];
      P[8 * j + 5] = after[j], memcpy(&Q[8 * j + 5], &sp[j], sizeof(g2_aff));
    }
  }
  if (run_delta) {
    memcpy(&P[4 * i_delta], fin->delta1, sizeof(g1_aff)), Q[4 * i_delta] = gen2;
    P[4 * i_delta + 1] = gen1, memcpy(&Q[4 * i_delta + 1], fin->delta2, sizeof(g2_aff));
  }
  for (size_t i : {i_c1, i_h1}) {
    memcpy(&Q[4 * i], ini->delta2, sizeof(g2_aff));
    memcpy(&Q[4 * i + 1], fin->delta2, sizeof(g2_aff));
  }

  DevMem<g1_aff> d_P;
  DevMem<g2_aff> d_Q;
  DevMem<int32_t> d_result;
  SyncOnExit drain{ctx->stream};
  HIPCHK(ctx, dev_alloc(d_P, P.size() * sizeof(g1_aff)));
  HIPCHK(ctx, dev_alloc(d_Q, Q.size() * sizeof(g2_aff)));
  HIPCHK(ctx, dev_alloc(d_result, nprod * sizeof(int32_t)));
  HIPCHK(ctx, hipMemcpyAsync(d_P.get(), P.data(), P.size() * sizeof(g1_aff), hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(d_Q.get(), Q.data(), Q.size() * sizeof(g2_aff), hipMemcpyHostToDevice, ctx->stream));
  // 3. the four sums, straight into their slots
  if (run_c1) {
    if ((rc = msm_host(ctx, z.data(), ini->pointsC1, nc1, d_P.get() + 4 * i_c1))) return rc;
    if ((rc = msm_host(ctx, z.data(), fin->pointsC1, nc1, d_P.get() + 4 * i_c1 + 1))) return rc;
  }
  if (run_h1) {
    if ((rc = msm_host(ctx, y.data(), ini->pointsH1, nh1, d_P.get() + 4 * i_h1))) return rc;
    if ((rc = msm_host(ctx, y.data(), fin->pointsH1, nh1, d_P.get() + 4 * i_h1 + 1))) return rc;
  }
  // 4. every product in one launch
  if ((rc = g16_pairing_products4(ctx, d_P.get(), d_Q.get(), (uint32_t)nprod, 2u, d_result.get()))) return rc;
  HIPCHK(ctx, hipMemcpyAsync(result.data(), d_result.get(), nprod * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));

  // 5. the verdicts
  int32_t* rel = out->relation;
  rel[G16_CHAIN_ELEMENTS] = elements ? 1 : 0;
  if (run_pok) {
    rel[G16_CHAIN_POK] = 1;
    for (size_t j = 0; j < count; ++j)
      if (!result[2 * j]) {
        rel[G16_CHAIN_POK] = 0, out->first_record[0] = j;
        break;
      }
  }
  if (run_step) {
    rel[G16_CHAIN_STEP] = 1;
    for (size_t j = 0; j < count; ++j)
      if (!result[2 * j + 1]) {
        rel[G16_CHAIN_STEP] = 0, out->first_record[1] = j;
        break;
      }
  }
  if (run_last) rel[G16_CHAIN_LAST] = !memcmp(fin->delta1, count ? (const void*)rec[count - 1].delta_after : ini->delta1, 64);
  if (run_delta) rel[G16_CHAIN_DELTA] = result[i_delta];
  if (run_c1) rel[G16_CHAIN_C1] = result[i_c1];
  if (run_h1) rel[G16_CHAIN_H1] = result[i_h1];
  for (int k = 0; k < G16_CHAIN_RELATIONS; ++k)
    if (rel[k] == 0) out->failed |= 1u << k;
  return G16_OK;
}

}  // namespace

extern "C" int32_t g16_key_contribute(g16_ctx* ctx, const g16_phase2_key* key, const void* d, const void* s,
                                      uint32_t flags, const void* challenge_g2, g16_phase2_out* out) {
  if (!ctx) return G16_EINVAL;
  auto bad = [&](const char* msg) {
    ctx->err = std::string("g16_key_contribute: ") + msg;
    return G16_EINVAL;
  };
  if (!key || !d || !s || !challenge_g2 || !out) return bad("null argument");
  if (!key->delta1 || !key->delta2 || (key->nc1 && !key->pointsC1) || (key->nh1 && !key->pointsH1))
    return bad("null key pointer");
  if (!out->delta1 || !out->delta2 || (key->nc1 && !out->pointsC1) || (key->nh1 && !out->pointsH1) || !out->record)
    return bad("null output pointer");
  if (flags != G16_SCALARS_MONT && flags != G16_SCALARS_STD) return bad("flags must be G16_SCALARS_MONT or G16_SCALARS_STD");
  if (key->nc1 >= (size_t(1) << 31) || key->nh1 >= (size_t(1) << 31)) return bad("array too long (must be < 2^31 points)");
  u256 d_std, s_std;
  if (!load_nonzero(d, flags == G16_SCALARS_MONT, d_std)) return bad("d must be non-zero and canonical (< r)");
  if (!load_nonzero(s, flags == G16_SCALARS_MONT, s_std)) return bad("s must be non-zero and canonical (< r)");
  if (all_zero(key->delta1, 64)) return bad("delta1 is the point at infinity");
  if (all_zero(key->delta2, 128)) return bad("delta2 is the point at infinity");
  if (all_zero(challenge_g2, 128)) return bad("the challenge is the point at infinity");
  CTX_ENTER(ctx);
  return key_contribute(ctx, key, d_std, s_std, challenge_g2, out);
}

extern "C" int32_t g16_contributions_verify(g16_ctx* ctx, const g16_phase2_key* initial, const g16_phase2_key* final_,
                                            const g16_contribution* records, const void* challenges_g2, size_t count,
                                            const void* c1_multipliers, const void* h1_multipliers,
                                            g16_chain_report* out) {
  if (!ctx) return G16_EINVAL;
  auto bad = [&](const char* msg) {
    ctx->err = std::string("g16_contributions_verify: ") + msg;
    return G16_EINVAL;
  };
  if (!initial || !final_ || !out || (count && (!records || !challenges_g2))) return bad("null argument");
  if (initial->nc1 != final_->nc1 || initial->nh1 != final_->nh1)
    return bad("the initial and the final key have other point counts (nc1, nh1)");
  for (const g16_phase2_key* k : {initial, final_})
    if (!k->delta1 || !k->delta2 || (k->nc1 && !k->pointsC1) || (k->nh1 && !k->pointsH1)) return bad("null key pointer");
  if ((initial->nc1 && !c1_multipliers) || (initial->nh1 && !h1_multipliers)) return bad("null multipliers");
  if (count >= (size_t(1) << 20)) return bad("too many records (count must be < 2^20)");
  if (initial->nc1 >= (size_t(1) << 27) || initial->nh1 >= (size_t(1) << 27)) return bad("array too long (must be < 2^27 points)");
  try {   // the record arrays and the widened multipliers live in host vectors: no exception may cross the C ABI
    std::vector<uint64_t> z, y;
    int32_t rc;
    if ((rc = g16_widen_multipliers(ctx, "g16_contributions_verify: c1", c1_multipliers, initial->nc1, z))) return rc;
    if ((rc = g16_widen_multipliers(ctx, "g16_contributions_verify: h1", h1_multipliers, initial->nh1, y))) return rc;
    memset(out, 0, sizeof *out);
    for (int k = 0; k < G16_CHAIN_RELATIONS; ++k) out->relation[k] = -1;
    out->first_record[0] = out->first_record[1] = NONE;
    for (int a = 0; a < G16_CHAIN_ARRAYS; ++a) out->first_infinity[a] = NONE;
    CTX_ENTER(ctx);
    return contributions_verify(ctx, initial, final_, records, challenges_g2, count, z, y, out);
  } catch (const std::bad_alloc&) {
    ctx->err = "out of host memory";
    return G16_ENOMEM;
  }
}
