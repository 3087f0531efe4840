// Audit of an untrusted proving key (include/g16hip.h, "key audit"): per-element checks of every point array and of
// the coefficient values, and the same-logarithm relations between the G1 and G2 halves of a key.  The reference
// asserts the curve equations while it loads a .zkey (mkG1 / mkG2, curves.nim:95-107); this is that and more, as one
// call that reports where a key fails instead of aborting.  Kernels: audit.cuh.
#include "audit.cuh"
#include "checker.hpp"

using namespace g16;

namespace {

// the constant of the curve equation
template <class C>
auto curve_b();
template <>
auto curve_b<G1>() {
  return Fp::add(Fp::dbl(Fp::one()), Fp::one());   // y^2 = x^3 + 3
}
template <>
auto curve_b<G2>() {
  g2_aff g;
  fp2_t b;
  g16_curve_consts_g2(&g, &b);
  return b;
}

void counts_reset(AuditCounts* c, int n) {
  for (int i = 0; i < n; ++i)
    for (int k = 0; k < 3; ++k) c[i].first_bad[k] = 0xffffffffu, c[i].bad_count[k] = 0;
}
void counts_out(const AuditCounts& c, size_t first_bad[3], size_t bad_count[3]) {
  for (int k = 0; k < 3; ++k) {
    first_bad[k] = c.first_bad[k] == 0xffffffffu ? NONE : (size_t)c.first_bad[k];
    bad_count[k] = c.bad_count[k];
  }
}

// one array: upload into the context's point staging buffer, one pass; the counts stay on the device (d_out)
template <class C>
int32_t audit_array(g16_ctx* ctx, const void* points, size_t n, AuditCounts* d_out) {
  if (!n) return G16_OK;
  if (int32_t rc = stage_points<C>(ctx, points, n)) return rc;
  constexpr int order = sizeof(typename C::Aff) == sizeof(g2_aff) ? 1 : 0;
  KLAUNCH(ctx, order ? "audit_points_g2" : "audit_points_g1", (audit_points<C, order>),
          (uint32_t)((n + AUDIT_BLOCK - 1) / AUDIT_BLOCK), AUDIT_BLOCK, order ? AUDIT_Q_WORDS * AUDIT_BLOCK * 4 : 0,
          (const typename C::Aff*)ctx->stage_p.p(),
          (uint32_t)n, curve_b<C>(), d_out);
  HIPCHK(ctx, hipGetLastError());
  return G16_OK;
}

template <class C>
int32_t points_audit(g16_ctx* ctx, const void* points, size_t n, size_t first_bad[3], size_t bad_count[3]) {
  if (!ctx) return G16_EINVAL;
  if (!first_bad || !bad_count || (n && !points) || n >= (size_t(1) << 31)) {
    ctx->err = "g16_points_audit: bad argument";
    return G16_EINVAL;
  }
  CTX_ENTER(ctx);
  int32_t rc;
  static_assert(sizeof(AuditCounts) <= STAGE_O_RESULT_BYTES, "stage_o's result slot");
  if ((rc = ensure_stage_o(ctx))) return rc;
  AuditCounts h;
  counts_reset(&h, 1);
  AuditCounts* d = (AuditCounts*)ctx->stage_o.p();
  HIPCHK(ctx, hipMemcpyAsync(d, &h, sizeof h, hipMemcpyHostToDevice, ctx->stream));
  if ((rc = audit_array<C>(ctx, points, n, d))) return rc;
  HIPCHK(ctx, hipMemcpyAsync(&h, d, sizeof h, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  counts_out(h, first_bad, bad_count);
  return G16_OK;
}

}  // namespace

// 16-byte multipliers -> 32-byte standard scalars; the index of a zero one goes to the error text
int32_t g16_widen_multipliers(g16_ctx* ctx, const char* who, const void* multipliers, size_t n, std::vector<uint64_t>& out) {
  try {
    out.assign(4 * n, 0);
  } catch (const std::bad_alloc&) {
    ctx->err = "out of host memory";
    return G16_ENOMEM;
  }
  for (size_t i = 0; i < n; ++i) {
    memcpy(&out[4 * i], (const char*)multipliers + 16 * i, 16);
    if (!(out[4 * i] | out[4 * i + 1])) {
      ctx->err = std::string(who) + ": multiplier " + std::to_string(i) + " is zero";
      return G16_EINVAL;
    }
  }
  return G16_OK;
}

// the element passes of `nsec` arrays and, for the key audit, of the coefficient values (g16_internal.hpp)
int32_t g16_audit_sections(g16_ctx* ctx, const g16_audit_section* sec, int nsec, size_t (*first_bad)[3],
                           size_t (*bad_count)[3], const g16_audit_coeffs* coeffs) {
  const int rows = nsec + (coeffs ? 1 : 0);
  if (rows > ElementPass::MAX) return fail(ctx, "g16_audit_sections", "too many arrays");
  AuditCounts h[ElementPass::MAX];
  counts_reset(h, rows);
  DevMem<AuditCounts> d_counts;
  DevMem<> d_coeffs;
  // every array uploaded whole, one after the other, through the context's staging buffer
  const int32_t rc = [&]() -> int32_t {
    HIPCHK(ctx, dev_alloc(d_counts, rows * sizeof(AuditCounts)));
    HIPCHK(ctx, hipMemcpyAsync(d_counts.get(), h, rows * sizeof(AuditCounts), hipMemcpyHostToDevice, ctx->stream));
    for (int s = 0; s < nsec; ++s)
      if (int32_t e = sec[s].group == 1 ? audit_array<G1>(ctx, sec[s].p, sec[s].n, d_counts.get() + s)
                                        : audit_array<G2>(ctx, sec[s].p, sec[s].n, d_counts.get() + s))
        return e;
    if (coeffs && coeffs->count) {
      const size_t bytes = coeffs->count * coeffs->stride;
      HIPCHK(ctx, dev_alloc(d_coeffs, bytes));
      HIPCHK(ctx, hipMemcpyAsync(d_coeffs.get(), coeffs->base, bytes, hipMemcpyHostToDevice, ctx->stream));
      KLAUNCH(ctx, "audit_coeffs", audit_coeffs, (uint32_t)((coeffs->count + 255) / 256), 256, 0,
              (const uint32_t*)d_coeffs.get(), (uint32_t)coeffs->count, (uint32_t)(coeffs->stride / 4),
              (uint32_t)(coeffs->value_offset / 4), d_counts.get() + nsec);
      HIPCHK(ctx, hipGetLastError());
    }
    HIPCHK(ctx, hipMemcpyAsync(h, d_counts.get(), rows * sizeof(AuditCounts), hipMemcpyDeviceToHost, ctx->stream));
    return G16_OK;
  }();
  // the one wait, on every path: before the two buffers go, and before a caller decides from the counts what may run next
  const hipError_t waited = hipStreamSynchronize(ctx->stream);
  if (rc) return rc;
  if (int32_t e = g16_hip_check(ctx->err, "hipStreamSynchronize(ctx->stream)", waited)) return e;
  for (int s = 0; s < rows; ++s) counts_out(h[s], first_bad[s], bad_count[s]);
  return G16_OK;
}

namespace {

// device scratch of the relations: a[3] | b[3] | result[3]
struct RelBuf {
  g1_aff a[3];
  g2_aff b[3];
  int32_t result[4];
};

// a[0] = sum z_i P_i, b[0] = sum z_i Q_i by the one-shot MSM (scalars: n x 32 B standard form, host)
int32_t relation_sums(g16_ctx* ctx, const void* g1_points, const void* g2_points, size_t n, const uint64_t* scalars,
                      RelBuf* d_rel) {
  int32_t rc;
  if ((rc = stage_scalars(ctx, scalars, n))) return rc;
  if ((rc = ensure(ctx, ctx->stage_p, n * sizeof(g2_aff)))) return rc;   // once, for both uploads
  if ((rc = staged_msm<G1>(ctx, ctx->stage_s.p(), G16_SCALARS_STD, g1_points, n, &d_rel->a[0]))) return rc;
  return staged_msm<G2>(ctx, ctx->stage_s.p(), G16_SCALARS_STD, g2_points, n, &d_rel->b[0]);
}

int32_t launch_relations(g16_ctx* ctx, RelBuf* d_rel, uint32_t first, uint32_t count) {
  KLAUNCH(ctx, "audit_relation", audit_relation, count, 64, 0, (const g1_aff*)d_rel->a + first,
          (const g2_aff*)d_rel->b + first, G1::neg(host_gen1()), host_gen2(), d_rel->result + first);
  HIPCHK(ctx, hipGetLastError());
  return G16_OK;
}

}  // namespace

extern "C" int32_t g16_points_audit_g1(g16_ctx* ctx, const void* points, size_t n, size_t first_bad[3],
                                       size_t bad_count[3]) {
  return points_audit<G1>(ctx, points, n, first_bad, bad_count);
}
extern "C" int32_t g16_points_audit_g2(g16_ctx* ctx, const void* points, size_t n, size_t first_bad[3],
                                       size_t bad_count[3]) {
  return points_audit<G2>(ctx, points, n, first_bad, bad_count);
}

extern "C" int32_t g16_points_pairs_check(g16_ctx* ctx, const void* g1_points, const void* g2_points, size_t n,
                                          const void* multipliers, int32_t* result) {
  if (!ctx) return G16_EINVAL;
  if (!result || (n && (!g1_points || !g2_points || !multipliers)) || n >= (size_t(1) << 27)) {
    ctx->err = "g16_points_pairs_check: bad argument";
    return G16_EINVAL;
  }
  std::vector<uint64_t> scalars;
  int32_t rc;
  if ((rc = g16_widen_multipliers(ctx, "g16_points_pairs_check", multipliers, n, scalars))) return rc;
  *result = 1;
  if (!n) return G16_OK;
  CTX_ENTER(ctx);
  DevMem<RelBuf> d_rel;
  SyncOnExit drain{ctx->stream};   // before d_rel goes
  HIPCHK(ctx, dev_alloc(d_rel, sizeof(RelBuf)));
  if ((rc = relation_sums(ctx, g1_points, g2_points, n, scalars.data(), d_rel.get()))) return rc;
  if ((rc = launch_relations(ctx, d_rel.get(), 0, 1))) return rc;
  HIPCHK(ctx, hipMemcpyAsync(result, d_rel->result, 4, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return G16_OK;
}

extern "C" int32_t g16_key_audit(g16_ctx* ctx, const g16_pkey_desc* d, const g16_vkey_desc* vk, const void* section4,
                                 size_t section4_bytes, const void* multipliers, g16_key_report* out) {
  return g16_key_audit_body(ctx, d, vk, section4, section4_bytes, multipliers, out);
}

// the whole of g16_key_audit, shared with g16_circuit_audit (circuit_audit.hip), whose report starts with the key's
int32_t g16_key_audit_body(g16_ctx* ctx, const g16_pkey_desc* d, const g16_vkey_desc* vk, const void* section4,
                           size_t section4_bytes, const void* multipliers, g16_key_report* out) {
  if (!ctx) return G16_EINVAL;
  if (!d || !out) {
    ctx->err = "g16_key_audit: null argument";
    return G16_EINVAL;
  }
  // the shape rules of g16_pkey_create*
  if (d->log2_domain > 27 || d->nvars == 0 || d->npubs + 1 > d->nvars || d->flavour > 1 || !d->pointsA1 ||
      !d->pointsB1 || !d->pointsB2 || !d->pointsH1 || (d->nvars - d->npubs - 1 > 0 && !d->pointsC1) || !d->alpha1 ||
      !d->beta1 || !d->delta1 || !d->beta2 || !d->delta2 || (d->ncoeffs && !d->coeffs) ||
      (section4 && (d->coeffs || d->ncoeffs))) {
    ctx->err = "g16_key_audit: bad proving-key description";
    return G16_EINVAL;
  }
  if (d->shard_count > 1) {
    ctx->err = "g16_key_audit: a sharded key description (audit the whole key: shard_count 0 or 1)";
    return G16_EINVAL;
  }
  if (multipliers && d->nvars >= (1u << 27)) {
    ctx->err = "g16_key_audit: too many wires for the batched relation (nvars < 2^27)";
    return G16_EINVAL;
  }
  if (vk && (vk->npubs != d->npubs || !vk->gamma2 || !vk->pointsIC)) {
    ctx->err = "g16_key_audit: the verification-key description does not belong to this key";
    return G16_EINVAL;
  }
  const size_t dom = size_t(1) << d->log2_domain;
  // the coefficient records: matrix, row and column on the host (as g16_pkey_create*), the values on the device
  const unsigned char* cbase = (const unsigned char*)d->coeffs;
  size_t ccount = d->ncoeffs, cstride = sizeof(g16_coeff), coff = offsetof(g16_coeff, value);
  if (section4) {
    uint32_t cnt;
    if (section4_bytes < 4 || (memcpy(&cnt, section4, 4), section4_bytes != 4 + (size_t)cnt * 44)) {
      ctx->err = "g16_key_audit: unexpected length of the coefficient section (4 + 44 * count bytes)";
      return G16_EINVAL;
    }
    cbase = (const unsigned char*)section4 + 4, ccount = cnt, cstride = 44, coff = 12;
  }
  if (ccount >= 0xffffffffu) {
    ctx->err = "g16_key_audit: too many coefficients";
    return G16_EINVAL;
  }
  for (size_t e = 0; e < ccount; ++e) {
    uint32_t mrc[3];
    memcpy(mrc, cbase + e * cstride, 12);
    if (mrc[0] > 1 || mrc[1] >= dom || mrc[2] >= d->nvars) {
      ctx->err = "g16_key_audit: coefficient entry " + std::to_string(e) + " out of range (matrix must be 0=A or 1=B)";
      return G16_EINVAL;
    }
  }
  std::vector<uint64_t> scalars;
  int32_t rc;
  if (multipliers && (rc = g16_widen_multipliers(ctx, "g16_key_audit", multipliers, d->nvars, scalars))) return rc;
  CTX_ENTER(ctx);

  const g16_audit_section sec[G16_AUDIT_SECTIONS - 1] = {
      {1, d->alpha1, 1}, {1, d->beta1, 1}, {1, d->delta1, 1}, {2, d->beta2, 1}, {2, vk ? vk->gamma2 : nullptr, vk ? 1u : 0u},
      {2, d->delta2, 1}, {1, vk ? vk->pointsIC : nullptr, vk ? (size_t)d->npubs + 1 : 0}, {1, d->pointsA1, d->nvars},
      {1, d->pointsB1, d->nvars}, {2, d->pointsB2, d->nvars}, {1, d->pointsC1, (size_t)d->nvars - d->npubs - 1},
      {1, d->pointsH1, dom}};
  const g16_audit_coeffs coeffs{cbase, ccount, cstride, coff};
  // The relations run only on sections whose every element passed: the sums and the Miller loops are defined for
  // canonical points of the curve and its order-r subgroup, nothing else.  Hence the wait of the pass between the two halves.
  DevMem<RelBuf> d_rel;
  SyncOnExit drain{ctx->stream};   // before d_rel goes
  HIPCHK(ctx, dev_alloc(d_rel, sizeof(RelBuf)));
  ElementPass pass;
  if ((rc = pass.run(ctx, KEY_ARRAYS, sec, &coeffs))) return rc;

  memset(out, 0, sizeof *out);
  pass.to_report(out->first_bad, out->bad_count);
  for (int s = 0; s < G16_AUDIT_SECTIONS; ++s) {
    static const uint32_t bit[3] = {G16_AUDIT_CANONICAL, G16_AUDIT_CURVE, G16_AUDIT_SUBGROUP};
    for (int k = 0; k < 3; ++k)
      if (out->bad_count[s][k]) out->failed |= bit[k];
  }
  out->spec_infinity = pass.infinite;   // (0,0) is on the curve: it fails no check and keeps no relation from running
  if (out->spec_infinity) out->failed |= G16_AUDIT_SPEC_INFINITY;
  bool run[3];
  relations_run(KEY_RELATIONS, ~pass.dirty, multipliers ? NEED_MULTIPLIERS : 0, run);
  int32_t* rel = out->relation;
  rel[0] = rel[1] = rel[2] = -1;
  if (run[0] || run[1] || run[2]) {
    // a relation that is not run keeps (0,0) on both sides: its workgroup multiplies two ones
    HIPCHK(ctx, hipMemsetAsync(d_rel.get(), 0, sizeof(RelBuf), ctx->stream));
    if (run[0] && (rc = relation_sums(ctx, d->pointsB1, d->pointsB2, d->nvars, scalars.data(), d_rel.get()))) return rc;
    const void* g1s[3] = {nullptr, d->beta1, d->delta1};
    const void* g2s[3] = {nullptr, d->beta2, d->delta2};
    for (int j = 1; j < 3; ++j) {
      if (!run[j]) continue;
      HIPCHK(ctx, hipMemcpyAsync(&d_rel->a[j], g1s[j], 64, hipMemcpyHostToDevice, ctx->stream));
      HIPCHK(ctx, hipMemcpyAsync(&d_rel->b[j], g2s[j], 128, hipMemcpyHostToDevice, ctx->stream));
    }
    if ((rc = launch_relations(ctx, d_rel.get(), 0, 3))) return rc;
    int32_t got[4];
    HIPCHK(ctx, hipMemcpyAsync(got, d_rel->result, sizeof got, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    for (int j = 0; j < 3; ++j)
      if (run[j]) rel[j] = got[j];
  }
  fold_report(KEY_RELATIONS, run, nullptr, 0, rel, nullptr, out->failed);
  return G16_OK;
}
