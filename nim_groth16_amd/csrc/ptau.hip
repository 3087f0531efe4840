// Phase-1 contribution (include/g16hip.h, "phase-1 contribution"): g16_ptau_contribute takes the powers of (tau, alpha,
// beta) to those of (t tau, a alpha, b beta); g16_ptau_verify checks such powers and a chain of records with the one-shot
// MSM and the four-pair product of the circuit audit.  Host layer only: the scalars c t^i are the geometric-sequence kernel of the
// setup (setup.hip), the scalings scale_each (scale_each.cuh), the element checks audit.hip.  Nothing is hashed or drawn.
#include <cstdlib>
#include <new>

#include "g16_internal.hpp"
#include "ec.cuh"

using namespace g16;

void g16_curve_consts_g2(void* gen2, void* twist_b);   // msm_g2_misc.hip: gen2 (128 B), twistCoeffB (64 B)

namespace {

constexpr uint32_t PTAU_MAX_POWER = 25;
constexpr size_t PTAU_CHUNK = size_t(1) << 22;   // points of a long array on the device at a time
constexpr size_t NONE = (size_t)-1;

// the chunk of this call: PTAU_CHUNK, or fewer points if G16_PTAU_CHUNK says so (the tests walk the chunk loop at power 3)
size_t ptau_chunk() {
  const char* e = getenv("G16_PTAU_CHUNK");
  const unsigned long long v = e ? strtoull(e, nullptr, 10) : 0;
  return v && v < PTAU_CHUNK ? (size_t)v : PTAU_CHUNK;
}
const char* const WHAT[3] = {"is not a canonical encoding", "is not on the curve", "is not in the order-r subgroup"};

bool all_zero(const void* p, size_t bytes) {   // bytes <= 128: one point
  static const unsigned char zeros[sizeof(g2_aff)] = {};
  return !memcmp(p, zeros, bytes);
}

// a 32-byte scalar of the caller, canonical and non-zero, to Montgomery form
bool load_nonzero(const void* p, bool mont, u256& mont_out) {
  u256 v;
  memcpy(&v, p, 32);
  if (!Fr::is_canonical(v) || Fr::is_zero(v)) return false;
  mont_out = mont ? v : Fr::to_mont(v);
  return true;
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
  auto bad = [&](const std::string& msg) {
    ctx->err = "g16_ptau_contribute: " + msg;
    return G16_EINVAL;
  };
  const size_t n = size_t(1) << ptau->power, n1 = 2 * n - 1;
  int32_t rc;
  // 1. the element passes, then the scan for (0,0)
  enum { NSEC = 6 };
  static const char* const names[NSEC] = {"ptau tauG1", "ptau tauG2", "ptau alphaTauG1", "ptau betaTauG1", "ptau betaG2",
                                          "challenges"};
  const g16_audit_section sec[NSEC] = {{1, ptau->tauG1, n1},    {2, ptau->tauG2, n}, {1, ptau->alphaTauG1, n},
                                       {1, ptau->betaTauG1, n}, {2, ptau->betaG2, 1}, {2, challenges, 3}};
  {
    size_t first_bad[NSEC][3], bad_count[NSEC][3];
    if ((rc = g16_audit_sections(ctx, sec, NSEC, first_bad, bad_count))) return rc;
    for (int s = 0; s < NSEC; ++s)
      for (int k = 0; k < 3; ++k) {
        if (!bad_count[s][k]) continue;
        std::string text = std::string(names[s]) + "[" + std::to_string(first_bad[s][k]) + "] " + WHAT[k];
        if (bad_count[s][k] > 1) text += " (and " + std::to_string(bad_count[s][k] - 1) + " more)";
        return bad(text);
      }
    for (int s = 0; s < NSEC; ++s) {
      const size_t psz = sec[s].group == 1 ? sizeof(g1_aff) : sizeof(g2_aff);
      for (size_t i = 0; i < sec[s].n; ++i)
        if (all_zero((const char*)sec[s].p + psz * i, psz))
          return bad(std::string(names[s]) + "[" + std::to_string(i) + "] is the point at infinity");
    }
  }

  // 2. the single points: s gen1 and x s gen1 for x = t, a, b; b betaG2 and x challenge_x
  const u256 one_std = Fr::from_mont(Fr::one());
  const g1_aff gen1{Fp::one(), Fp::dbl(Fp::one())};
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
  const g1_aff gen1{Fp::one(), Fp::dbl(Fp::one())};
  g2_aff gen2;
  {
    fp2_t twist_b;
    g16_curve_consts_g2(&gen2, &twist_b);
  }
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
  enum { NA = G16_PTAU_REPORT_ARRAYS };
  const g16_audit_section sec[NA] = {
      {1, ptau->tauG1, n1},       {2, ptau->tauG2, n},        {1, ptau->alphaTauG1, n},   {1, ptau->betaTauG1, n},
      {2, ptau->betaG2, 1},       {1, r1[0].data(), count},   {1, r1[1].data(), count},   {1, r1[2].data(), count},
      {2, r2[0].data(), count},   {2, r2[1].data(), count},   {1, gs.data(), 3 * count},  {1, gsx.data(), 3 * count},
      {2, spx.data(), 3 * count}, {2, challenges, 3 * count}};
  if ((rc = g16_audit_sections(ctx, sec, NA, out->first_bad, out->bad_count))) return rc;
  bool clean[NA], elements = true;
  for (int a = 0; a < NA; ++a) {
    clean[a] = !(out->bad_count[a][0] | out->bad_count[a][1] | out->bad_count[a][2]);
    const size_t psz = sec[a].group == 1 ? sizeof(g1_aff) : sizeof(g2_aff);
    for (size_t i = 0; i < sec[a].n; ++i)
      if (all_zero((const char*)sec[a].p + psz * i, psz)) {
        out->first_infinity[a] = i;
        clean[a] = false;
        break;
      }
    elements = elements && clean[a];
  }
  auto all_clean = [&](int from, int to) {
    for (int a = from; a <= to; ++a)
      if (!clean[a]) return false;
    return true;
  };
  const bool tau_ok = clean[G16_PTAU_TAU_G1] && clean[G16_PTAU_TAU_G2];
  const bool run_alpha = clean[G16_PTAU_ALPHA_TAU_G1] && clean[G16_PTAU_TAU_G2];
  const bool run_beta = clean[G16_PTAU_BETA_TAU_G1] && clean[G16_PTAU_TAU_G2];
  const bool run_bg2 = clean[G16_PTAU_BETA_TAU_G1] && clean[G16_PTAU_BETA_G2];
  const bool run_pok = chain && all_clean(G16_PTAUV_G1_S, G16_PTAUV_CHALLENGES);
  const bool run_step = run_pok && all_clean(G16_PTAUV_REC_TAU_G1, G16_PTAUV_REC_BETA_G2);
  const bool run_last = chain && all_clean(G16_PTAU_TAU_G1, G16_PTAUV_REC_BETA_G2);

  // 2. the products, each e(P0, Q0) e(-P1, Q1): TAU_G1, TAU_G2, ALPHA, BETA, BETA_G2, then per record three POK and five
  //    STEP.  Pairs 2 and 3, and every product that is not run, keep (0,0) and contribute one.
  enum { I_TAU1 = 0, I_TAU2, I_ALPHA, I_BETA, I_BG2, FIXED };
  const size_t nprod = FIXED + 8 * count;
  std::vector<g1_aff> P(4 * nprod);
  std::vector<g2_aff> Q(4 * nprod);
  std::vector<int32_t> result(nprod, 0);
  memset(P.data(), 0, P.size() * sizeof(g1_aff));
  memset(Q.data(), 0, Q.size() * sizeof(g2_aff));
  const g1_aff* tau1 = (const g1_aff*)ptau->tauG1;
  const g2_aff* tau2 = (const g2_aff*)ptau->tauG2;
  const g2_aff* ch = (const g2_aff*)challenges;
  auto g1_at = [](const void* p, size_t i) { g1_aff v; memcpy(&v, (const char*)p + 64 * i, 64); return v; };
  auto g2_at = [](const void* p, size_t i) { g2_aff v; memcpy(&v, (const char*)p + 128 * i, 128); return v; };
  if (tau_ok) {
    Q[4 * I_TAU1] = g2_at(tau2, 1), Q[4 * I_TAU1 + 1] = gen2;
    P[4 * I_TAU2] = g1_at(tau1, 1), P[4 * I_TAU2 + 1] = gen1;
  }
  if (run_alpha) Q[4 * I_ALPHA] = g2_at(tau2, 1), Q[4 * I_ALPHA + 1] = gen2;
  if (run_beta) Q[4 * I_BETA] = g2_at(tau2, 1), Q[4 * I_BETA + 1] = gen2;
  if (run_bg2) {
    P[4 * I_BG2] = g1_at(ptau->betaTauG1, 0), Q[4 * I_BG2] = gen2;
    P[4 * I_BG2 + 1] = gen1, Q[4 * I_BG2 + 1] = g2_at(ptau->betaG2, 0);
  }
  for (size_t j = 0; j < count; ++j) {
    const size_t base = 4 * (FIXED + 8 * j);
    for (int x = 0; x < 3; ++x) {
      const size_t k = 3 * j + x;
      if (run_pok) {
        P[base + 4 * x] = gs[k], Q[base + 4 * x] = spx[k];
        P[base + 4 * x + 1] = gsx[k], Q[base + 4 * x + 1] = g2_at(ch, k);
      }
      if (run_step) {   // the G1 value that x moves: tauG1 by t, alphaG1 by a, betaG1 by b
        const size_t q = base + 4 * (3 + x);
        P[q] = j ? r1[x][j - 1] : gen1, Q[q] = spx[k];
        P[q + 1] = r1[x][j], Q[q + 1] = g2_at(ch, k);
      }
    }
    if (run_step)
      for (int y = 0; y < 2; ++y) {   // tauG2 moves by t (pok 0), betaG2 by b (pok 2)
        const size_t q = base + 4 * (6 + y), k = 3 * j + (y ? 2 : 0);
        P[q] = gsx[k], Q[q] = j ? r2[y][j - 1] : gen2;
        P[q + 1] = gs[k], Q[q + 1] = r2[y][j];
      }
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
  // 3. the sums: the multipliers once, every array at the point offsets 0 and 1
  const size_t m = n1 - 1;
  if ((rc = ensure(ctx, ctx->stage_s, m * 32))) return rc;
  if ((rc = ensure(ctx, ctx->stage_p, n1 * sizeof(g1_aff)))) return rc;   // = n G2 points and more
  HIPCHK(ctx, hipMemcpyAsync(ctx->stage_s.p(), z.data(), m * 32, hipMemcpyHostToDevice, ctx->stream));
  auto sums_g1 = [&](const void* pts, size_t have, size_t terms, g1_aff* d_out) -> int32_t {
    HIPCHK(ctx, hipMemcpyAsync(ctx->stage_p.p(), pts, have * sizeof(g1_aff), hipMemcpyHostToDevice, ctx->stream));
    for (int off = 0; off < 2; ++off)
      if (int32_t e = msm_device<G1>(ctx, ctx->stage_s.p(), G16_SCALARS_STD, (const g1_aff*)ctx->stage_p.p() + off, terms,
                                     d_out + off, nullptr, 0))
        return e;
    return G16_OK;
  };
  if (tau_ok) {
    if ((rc = sums_g1(ptau->tauG1, n1, m, d_P.get() + 4 * I_TAU1))) return rc;
    HIPCHK(ctx, hipMemcpyAsync(ctx->stage_p.p(), ptau->tauG2, n * sizeof(g2_aff), hipMemcpyHostToDevice, ctx->stream));
    for (int off = 0; off < 2; ++off)
      if ((rc = msm_device<G2>(ctx, ctx->stage_s.p(), G16_SCALARS_STD, (const g2_aff*)ctx->stage_p.p() + off, n - 1,
                               d_Q.get() + 4 * I_TAU2 + off, nullptr, 0)))
        return rc;
  }
  if (run_alpha && (rc = sums_g1(ptau->alphaTauG1, n, n - 1, d_P.get() + 4 * I_ALPHA))) return rc;
  if (run_beta && (rc = sums_g1(ptau->betaTauG1, n, n - 1, d_P.get() + 4 * I_BETA))) return rc;
  // 4. every product in one launch
  if ((rc = g16_pairing_products4(ctx, d_P.get(), d_Q.get(), (uint32_t)nprod, 2u, d_result.get()))) return rc;
  HIPCHK(ctx, hipMemcpyAsync(result.data(), d_result.get(), nprod * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));

  // 5. the verdicts
  int32_t* rel = out->relation;
  rel[G16_PTAUV_ELEMENTS] = elements ? 1 : 0;
  if (tau_ok) {
    rel[G16_PTAUV_FIRST] = !memcmp(ptau->tauG1, &gen1, 64) && !memcmp(ptau->tauG2, &gen2, 128);
    rel[G16_PTAUV_TAU_G1] = result[I_TAU1], rel[G16_PTAUV_TAU_G2] = result[I_TAU2];
  }
  if (run_alpha) rel[G16_PTAUV_ALPHA] = result[I_ALPHA];
  if (run_beta) rel[G16_PTAUV_BETA] = result[I_BETA];
  if (run_bg2) rel[G16_PTAUV_BETA_G2] = result[I_BG2];
  for (int which = 0; which < 2; ++which) {   // POK: products 0..2 of a record, STEP: 3..7
    if (!(which ? run_step : run_pok)) continue;
    const int r = which ? G16_PTAUV_STEP : G16_PTAUV_POK;
    rel[r] = 1;
    for (size_t j = 0; j < count && rel[r]; ++j)
      for (int q = which ? 3 : 0; q < (which ? 8 : 3); ++q)
        if (!result[FIXED + 8 * j + q]) {
          rel[r] = 0, out->first_record[which] = j;
          break;
        }
  }
  if (run_last) {
    const void* last[5] = {count ? (const void*)rec[count - 1].tauG1 : &gen1, count ? (const void*)rec[count - 1].alphaG1 : &gen1,
                           count ? (const void*)rec[count - 1].betaG1 : &gen1, count ? (const void*)rec[count - 1].tauG2 : &gen2,
                           count ? (const void*)rec[count - 1].betaG2 : &gen2};
    rel[G16_PTAUV_LAST] = !memcmp((const char*)ptau->tauG1 + 64, last[0], 64) && !memcmp(ptau->alphaTauG1, last[1], 64) &&
                          !memcmp(ptau->betaTauG1, last[2], 64) && !memcmp((const char*)ptau->tauG2 + 128, last[3], 128) &&
                          !memcmp(ptau->betaG2, last[4], 128);
  }
  for (int k = 0; k < G16_PTAU_RELATIONS; ++k)
    if (rel[k] == 0) out->failed |= 1u << k;
  return G16_OK;
}

}  // namespace

static_assert(sizeof(g16_ptau_contribution) == 1216, "a phase-1 record is 1216 bytes");

extern "C" int32_t g16_ptau_contribute(g16_ctx* ctx, const g16_ptau_desc* ptau, const void* t, const void* a, const void* b,
                                       const void* s3, uint32_t flags, const void* challenges_g2, g16_ptau_out* out,
                                       g16_ptau_contribution* record) {
  if (!ctx) return G16_EINVAL;
  auto bad = [&](const char* msg) {
    ctx->err = std::string("g16_ptau_contribute: ") + msg;
    return G16_EINVAL;
  };
  if (!ptau || !t || !a || !b || !s3 || !challenges_g2 || !out || !record) return bad("null argument");
  if (!ptau->tauG1 || !ptau->tauG2 || !ptau->alphaTauG1 || !ptau->betaTauG1 || !ptau->betaG2) return bad("null ptau pointer");
  if (!out->tauG1 || !out->tauG2 || !out->alphaTauG1 || !out->betaTauG1 || !out->betaG2) return bad("null output pointer");
  if (flags != G16_SCALARS_MONT && flags != G16_SCALARS_STD) return bad("flags must be G16_SCALARS_MONT or G16_SCALARS_STD");
  if (ptau->power == 0 || ptau->power > PTAU_MAX_POWER) return bad("power out of range (must be 1..25)");
  const bool mont = flags == G16_SCALARS_MONT;
  u256 x[3], sx[3];
  if (!load_nonzero(t, mont, x[0])) return bad("t must be non-zero and canonical (< r)");
  if (!load_nonzero(a, mont, x[1])) return bad("a must be non-zero and canonical (< r)");
  if (!load_nonzero(b, mont, x[2])) return bad("b must be non-zero and canonical (< r)");
  for (int j = 0; j < 3; ++j)
    if (!load_nonzero((const char*)s3 + 32 * j, mont, sx[j])) return bad("s must be non-zero and canonical (< r), all three");
  CTX_ENTER(ctx);
  try {   // the error texts are strings: no exception may cross the C ABI
    return ptau_contribute(ctx, ptau, x, sx, challenges_g2, out, record);
  } catch (const std::bad_alloc&) {
    ctx->err = "out of host memory";
    return G16_ENOMEM;
  }
}

extern "C" int32_t g16_ptau_verify(g16_ctx* ctx, const g16_ptau_desc* ptau, const g16_ptau_contribution* records,
                                   const void* challenges_g2, size_t count, const void* multipliers, g16_ptau_report* out) {
  if (!ctx) return G16_EINVAL;
  auto bad = [&](const char* msg) {
    ctx->err = std::string("g16_ptau_verify: ") + msg;
    return G16_EINVAL;
  };
  if (!ptau || !multipliers || !out || (count && (!records || !challenges_g2))) return bad("null argument");
  if (!ptau->tauG1 || !ptau->tauG2 || !ptau->alphaTauG1 || !ptau->betaTauG1 || !ptau->betaG2) return bad("null ptau pointer");
  if (ptau->power == 0 || ptau->power > PTAU_MAX_POWER) return bad("power out of range (must be 1..25)");
  if (count >= (size_t(1) << 16)) return bad("too many records (count must be < 2^16)");
  try {   // the record arrays and the widened multipliers live in host vectors: no exception may cross the C ABI
    std::vector<uint64_t> z;
    if (int32_t rc = g16_widen_multipliers(ctx, "g16_ptau_verify", multipliers, (size_t(2) << ptau->power) - 2, z)) return rc;
    memset(out, 0, sizeof *out);
    for (int k = 0; k < G16_PTAU_RELATIONS; ++k) out->relation[k] = -1;
    out->first_record[0] = out->first_record[1] = NONE;
    for (int a = 0; a < G16_PTAU_REPORT_ARRAYS; ++a) out->first_infinity[a] = NONE;
    CTX_ENTER(ctx);
    return ptau_verify(ctx, ptau, records, challenges_g2, count, records != nullptr, z, out);
  } catch (const std::bad_alloc&) {
    ctx->err = "out of host memory";
    return G16_ENOMEM;
  }
}
