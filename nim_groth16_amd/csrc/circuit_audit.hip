// Circuit audit (include/g16hip.h, "circuit audit"): does an untrusted proving key belong to a given R1CS and a given
// powers of tau?  The caller's multipliers z are treated as a witness.  buildABC over the key's coefficients and over
// the R1CS must give the same vectors; an inverse NTT turns A z into the coefficients of sum_i z_i A_i(X), whose MSM
// against the powers tau^k gen1 must be the prover's own MSM(z, pointsA1); pointsB1 / B2 / C1 / IC / H1 follow the same
// way, the last three through one pairing product each.  Nothing here is new arithmetic: the sparse products are
// spmv.hip, the transforms ntt.hip, the sums the one-shot MSM, the element checks audit.hip, all in the shape of a checker
// (checker.hpp).  Kernels: circuit_audit.cuh.
#include "circuit_audit.cuh"
#include "checker.hpp"

using namespace g16;

// `count` pairing products of four pairs each, one workgroup per product (pairing_product<4>, circuit_audit.cuh); shared
// with every ProductTable (checker.hpp)
int32_t g16_pairing_products4(g16_ctx* ctx, const void* d_P, const void* d_Q, uint32_t count, uint32_t neg_mask,
                              int32_t* d_result) {
  if (!count) return G16_OK;
  KLAUNCH(ctx, "pairing_product4", pairing_product<4>, count, 64, 0, (const g1_aff*)d_P, (const g2_aff*)d_Q, neg_mask,
          d_result);
  HIPCHK(ctx, hipGetLastError());
  return G16_OK;
}

namespace {

// device scratch of the point relations that compare two sums.  C1, IC and H1 are rows 0, 1, 2 of a ProductTable: C1 and
// IC { MSM(z|., points), R1, R2, R3 } x { delta2 / gamma2, gen2, gen2, gen2 }, H1 { MSM(y, pointsH1), MSM(c, tauG1) } x
// { delta2, gen2 }
struct SumBuf {
  g1_aff lhs1[2], rhs1[2];   // A1, B1: MSM(z, points) and MSM(coef, tauG1)
  g2_aff lhs2, rhs2;         // B2
};

uint32_t ceil_log2(uint64_t x) {
  uint32_t k = 0;
  while ((uint64_t(1) << k) < x) ++k;
  return k;
}

inline uint32_t grid_of(size_t n) { return (uint32_t)((n + CA_BLOCK - 1) / CA_BLOCK); }

// everything g16_circuit_audit rejects itself, before anything is queued (the key description's own shape rules are
// g16_key_audit's, which runs first and queues nothing before it has checked them)
int32_t validate(g16_ctx* ctx, const g16_pkey_desc* d, const g16_r1cs_desc* r, const g16_ptau_desc* t,
                 const void* wire_multipliers, const void* h_multipliers, g16_circuit_report* out) {
  static const char who[] = "g16_circuit_audit";
  if (!d || !r || !t || !wire_multipliers || !h_multipliers || !out) return fail(ctx, who, "null argument");
  if (!t->tauG1 || !t->tauG2 || !t->alphaTauG1 || !t->betaTauG1 || !t->betaG2) return fail(ctx, who, "null ptau section");
  for (int k = 0; k < 3; ++k)
    if (r->nnz[k] && (!r->row[k] || !r->col[k] || !r->val[k])) return fail(ctx, who, "null matrix pointer");
  if (d->shard_count > 1) return fail(ctx, who, "a sharded key description (audit the whole key: shard_count 0 or 1)");
  if (d->log2_domain > 27 || d->nvars == 0 || d->nvars >= (1u << 27)) return fail(ctx, who, "bad proving-key description");
  if (r->nvars != d->nvars || r->npubs != d->npubs)
    return fail(ctx, who, "the r1cs has other wire counts (nvars, npubs) than the key");
  if (r->flavour != d->flavour) return fail(ctx, who, "the flavour of the r1cs description is not the key's");
  if (r->flags != G16_SCALARS_MONT && r->flags != G16_SCALARS_STD)
    return fail(ctx, who, "r1cs flags must be G16_SCALARS_MONT or _STD");
  if (ceil_log2((uint64_t)r->nconstraints + r->npubs + 1) != d->log2_domain)
    return fail(ctx, who, "ceilingLog2(nconstraints + npubs + 1) of the r1cs is not the key's log2_domain");
  if (t->power < d->log2_domain + 1 || t->power > 28)
    return fail(ctx, who, "the powers of tau are too short: power >= log2_domain + 1 is needed (tau^(2n-1); and power <= 28)");
  for (int k = 0; k < 3; ++k)
    for (size_t i = 0; i < r->nnz[k]; ++i) {
      if (r->row[k][i] >= r->nconstraints || r->col[k][i] >= r->nvars)
        return fail(ctx, who, "r1cs matrix " + std::to_string(k) + " entry " + std::to_string(i) + " out of range");
      u256 v;
      memcpy(&v, (const char*)r->val[k] + 32 * i, 32);
      if (!Fr::is_canonical(v))
        return fail(ctx, who, "r1cs matrix " + std::to_string(k) + " entry " + std::to_string(i) + ": value is not canonical (>= r)");
    }
  return G16_OK;
}

using SpMat = Building<g16_spmat, g16_spmat_destroy>;

// the key's A and B as buildABC sees them (bin_coefficients, pkey.hip); ranges were checked by the key audit
int32_t key_matrix(g16_ctx* ctx, const g16_pkey_desc* d, const void* section4, SpMat& out) {
  const unsigned char* base = (const unsigned char*)d->coeffs;
  size_t count = d->ncoeffs, stride = sizeof(g16_coeff), voff = offsetof(g16_coeff, value);
  bool r2 = false;
  if (section4) {
    uint32_t cnt;
    memcpy(&cnt, section4, 4);
    base = (const unsigned char*)section4 + 4, count = cnt, stride = 44, voff = 12, r2 = true;
  }
  std::vector<uint32_t> vrow(count ? count : 1);
  for (size_t e = 0; e < count; ++e) {
    uint32_t mr[2];
    memcpy(mr, base + e * stride, 8);
    vrow[e] = 2 * mr[1] + mr[0];
  }
  g16_spmat* built = nullptr;
  const int32_t rc = g16_spmat_create(ctx, 2, 1u << d->log2_domain, count, vrow.data(), 4,
                                      (const uint32_t*)(count ? base + 8 : nullptr), stride, count ? base + voff : nullptr,
                                      stride, &built, r2);
  out.reset(built);
  return rc;
}

// the R1CS: `ab` = A (with snarkjs's dummy entries (nconstraints + i, wire i, 1), i <= npubs) and B as one two-matrix
// product like the key's; `c` = C in the A slot of a second one
int32_t r1cs_matrices(g16_ctx* ctx, const g16_r1cs_desc* r, uint32_t log2_dom, SpMat& ab, SpMat& c) {
  const bool mont = r->flags == G16_SCALARS_MONT;
  const size_t nab = r->nnz[0] + r->nnz[1] + r->npubs + 1;
  std::vector<uint32_t> vrow(nab), col(nab);
  std::vector<u256> val(nab);
  size_t e = 0;
  auto take = [&](int k, uint32_t slot, std::vector<uint32_t>& vr, std::vector<uint32_t>& cl, std::vector<u256>& vl,
                  size_t& at) {
    for (size_t i = 0; i < r->nnz[k]; ++i, ++at) {
      vr[at] = 2 * r->row[k][i] + slot, cl[at] = r->col[k][i];
      memcpy(&vl[at], (const char*)r->val[k] + 32 * i, 32);
      if (!mont) vl[at] = Fr::to_mont(vl[at]);
    }
  };
  take(0, 0, vrow, col, val, e);
  take(1, 1, vrow, col, val, e);
  for (uint32_t i = 0; i <= r->npubs; ++i, ++e) vrow[e] = 2 * (r->nconstraints + i), col[e] = i, val[e] = Fr::one();
  g16_spmat* built = nullptr;
  int32_t rc = g16_spmat_create(ctx, 2, 1u << log2_dom, nab, vrow.data(), 4, col.data(), 4, val.data(), 32, &built);
  ab.reset(built);
  if (rc) return rc;
  const size_t nc = r->nnz[2];
  std::vector<uint32_t> crow(nc ? nc : 1), ccol(nc ? nc : 1);
  std::vector<u256> cval(nc ? nc : 1);
  e = 0;
  take(2, 0, crow, ccol, cval, e);
  built = nullptr;
  rc = g16_spmat_create(ctx, 2, 1u << log2_dom, nc, crow.data(), 4, ccol.data(), 4, cval.data(), 32, &built);
  c.reset(built);
  return rc;
}

// a host point array into device memory of its own
template <class T>
int32_t upload_points(g16_ctx* ctx, DevMem<T>& dst, const void* src, size_t count) {
  HIPCHK(ctx, dev_alloc(dst, count * sizeof(T)));
  HIPCHK(ctx, hipMemcpyAsync(dst.get(), src, count * sizeof(T), hipMemcpyHostToDevice, ctx->stream));
  return G16_OK;
}

int32_t circuit_audit(g16_ctx* ctx, const g16_pkey_desc* d, const g16_vkey_desc* vk, const void* section4,
                      const g16_r1cs_desc* r, const g16_ptau_desc* t, const void* wire_multipliers,
                      const void* h_multipliers, g16_circuit_report* out) {
  const uint32_t L = d->log2_domain, nv = d->nvars, npubs = d->npubs;
  const size_t n = size_t(1) << L, npriv = (size_t)nv - npubs - 1;
  const bool snarkjs = d->flavour == G16_FLAVOUR_SNARKJS;
  int32_t rc;

  // 1. the element passes over what is read of the five ptau arrays
  const g16_audit_section psec[G16_PTAU_SECTIONS] = {
      {1, t->tauG1, 2 * n}, {2, t->tauG2, n}, {1, t->alphaTauG1, n}, {1, t->betaTauG1, n}, {2, t->betaG2, 1}};
  ElementPass pass;
  if ((rc = pass.run(ctx, CIRCUIT_PTAU_ARRAYS, psec))) return rc;
  pass.to_report(out->ptau_first_bad, out->ptau_bad_count);
  if (pass.dirty) out->failed |= G16_CIRCUIT_PTAU;
  bool run[G16_CIRCUIT_RELATIONS];
  relations_run(CIRCUIT_RELATIONS, ~(dirty_mask(out->key.bad_count, G16_AUDIT_SECTIONS) | pass.dirty << CIRCUIT_PTAU_BIT),
                vk ? NEED_VK : 0, run);
  int32_t* rel = out->relation;   // every one -1: not run

  // 2. SPEC: bytes on the host
  const g1_aff gen1 = host_gen1();
  const g2_aff gen2 = host_gen2();
  if (run[G16_REL_SPEC])
    rel[G16_REL_SPEC] = !memcmp(d->alpha1, t->alphaTauG1, 64) && !memcmp(d->beta1, t->betaTauG1, 64) &&
                        !memcmp(d->beta2, t->betaG2, 128) && !memcmp(t->tauG1, &gen1, 64) && !memcmp(t->tauG2, &gen2, 128);

  // 3. owners first, the drain of the stream that uses them last (released in reverse order)
  SpMat m_key, m_ab, m_c;
  DevMem<uint4> d_z16, d_y16;
  DevMem<u256> d_z, d_key, d_ab, d_cc, d_sum, d_h, d_ystd;
  DevMem<uint32_t> d_first;
  DevMem<g1_aff> d_tau1, d_alpha, d_beta;
  DevMem<g2_aff> d_tau2;
  DevMem<SumBuf> d_pb;
  ProductTable pt(3);
  SyncOnExit drain{ctx->stream};
  if ((rc = key_matrix(ctx, d, section4, m_key))) return rc;
  if ((rc = r1cs_matrices(ctx, r, L, m_ab, m_c))) return rc;
  HIPCHK(ctx, dev_alloc(d_z16, (size_t)nv * 16));
  HIPCHK(ctx, dev_alloc(d_y16, n * 16));
  HIPCHK(ctx, dev_alloc(d_z, 3 * (size_t)nv * 32));
  HIPCHK(ctx, dev_alloc(d_key, 6 * n * 32));
  HIPCHK(ctx, dev_alloc(d_ab, 6 * n * 32));
  HIPCHK(ctx, dev_alloc(d_cc, 6 * n * 32));
  HIPCHK(ctx, dev_alloc(d_sum, 2 * n * 32));
  HIPCHK(ctx, dev_alloc(d_h, 2 * n * 32));
  HIPCHK(ctx, dev_alloc(d_ystd, n * 32));
  HIPCHK(ctx, dev_alloc(d_first, 8));
  HIPCHK(ctx, dev_alloc(d_pb, sizeof(SumBuf)));
  HIPCHK(ctx, hipMemsetAsync(d_pb.get(), 0, sizeof(SumBuf), ctx->stream));
  HIPCHK(ctx, hipMemsetAsync(d_first.get(), 0xff, 8, ctx->stream));
  HIPCHK(ctx, hipMemsetAsync(d_key.get(), 0, 6 * n * 32, ctx->stream));
  HIPCHK(ctx, hipMemsetAsync(d_ab.get(), 0, 6 * n * 32, ctx->stream));
  HIPCHK(ctx, hipMemsetAsync(d_cc.get(), 0, 6 * n * 32, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(d_z16.get(), wire_multipliers, (size_t)nv * 16, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(d_y16.get(), h_multipliers, n * 16, hipMemcpyHostToDevice, ctx->stream));
  u256 *z_all = d_z.get(), *z_pub = z_all + nv, *z_priv = z_pub + nv;
  KLAUNCH(ctx, "circuit_widen", widen_mask, grid_of(nv), CA_BLOCK, 0, (const uint4*)d_z16.get(), nv, npubs, z_all, z_pub,
          z_priv);
  HIPCHK(ctx, hipGetLastError());

  // 4. the products: [pub: A | B | (C)] [priv: A | B | (C)], Montgomery.  The multipliers are standard-form scalars.
  u256* zs[2] = {z_pub, z_priv};
  for (int h = 0; h < 2; ++h) {
    if (run[G16_REL_COEFFS_A] && (rc = g16_spmat_apply(ctx, m_key.get(), zs[h], 0, d_key.get() + 3 * n * h, false)))
      return rc;
    if ((rc = g16_spmat_apply(ctx, m_ab.get(), zs[h], 0, d_ab.get() + 3 * n * h, false))) return rc;
    if ((rc = g16_spmat_apply(ctx, m_c.get(), zs[h], 0, d_cc.get() + 3 * n * h, false))) return rc;
  }
  // 5. COEFFS_A / COEFFS_B: the first row where the key's product and the R1CS's differ
  if (run[G16_REL_COEFFS_A])
    for (int h = 0; h < 2; ++h)
      for (int k = 0; k < 2; ++k) {
        KLAUNCH(ctx, "circuit_compare", vec_first_mismatch, grid_of(n), CA_BLOCK, 0,
                (const u256*)d_key.get() + 3 * n * h + n * k, (const u256*)d_ab.get() + 3 * n * h + n * k, (uint32_t)n,
                d_first.get() + k);
        HIPCHK(ctx, hipGetLastError());
      }
  uint32_t first[2] = {0xffffffffu, 0xffffffffu};
  HIPCHK(ctx, hipMemcpyAsync(first, d_first.get(), 8, hipMemcpyDeviceToHost, ctx->stream));

  // 6. values on the domain -> coefficients, in place: A, B, C over z|pub and z|priv; A z and B z by linearity
  for (int h = 0; h < 2; ++h) {
    for (int k = 0; k < 2; ++k)
      if ((rc = g16_ntt_device(ctx, d_ab.get() + 3 * n * h + n * k, d_ab.get() + 3 * n * h + n * k, L, 1))) return rc;
    if ((rc = g16_ntt_device(ctx, d_cc.get() + 3 * n * h, d_cc.get() + 3 * n * h, L, 1))) return rc;
  }
  for (int k = 0; k < 2; ++k) {
    KLAUNCH(ctx, "circuit_add", vec_add, grid_of(n), CA_BLOCK, 0, (const u256*)d_ab.get() + n * k,
            (const u256*)d_ab.get() + 3 * n + n * k, (uint32_t)n, d_sum.get() + n * k);
    HIPCHK(ctx, hipGetLastError());
  }
  // ... and the H side
  KLAUNCH(ctx, "circuit_h_scatter", h_scatter, grid_of(n), CA_BLOCK, 0, (const uint4*)d_y16.get(), (uint32_t)n,
          snarkjs ? 1u : 0u, d_h.get(), d_ystd.get());
  HIPCHK(ctx, hipGetLastError());
  if (snarkjs && (rc = g16_ntt_device(ctx, d_h.get(), d_h.get(), L + 1, 1))) return rc;

  // 7. the sums
  SumBuf* pb = d_pb.get();
  // C1 over z|priv (row 0), IC over z|pub (row 1).  No private wire: both sides are infinity, nothing to run.
  const bool pair4[2] = {run[G16_REL_C1] && npriv > 0, run[G16_REL_IC]};
  for (int j = 0; j < 2; ++j)
    if (pair4[j]) {
      pt.set(j, 0, nullptr, j == 0 ? d->delta2 : vk->gamma2);
      for (int k = 1; k < 4; ++k) pt.set(j, k, nullptr, &gen2);
    }
  if (run[G16_REL_H1]) pt.set(2, 0, nullptr, d->delta2), pt.set(2, 1, nullptr, &gen2);
  if ((rc = pt.upload(ctx))) return rc;
  const bool need_tau1 = run[G16_REL_A1] || run[G16_REL_B1] || run[G16_REL_C1] || run[G16_REL_IC] || run[G16_REL_H1];
  if (need_tau1 && (rc = upload_points(ctx, d_tau1, t->tauG1, 2 * n))) return rc;
  if (run[G16_REL_B2] && (rc = upload_points(ctx, d_tau2, t->tauG2, n))) return rc;
  if ((run[G16_REL_C1] || run[G16_REL_IC]) &&
      ((rc = upload_points(ctx, d_alpha, t->alphaTauG1, n)) || (rc = upload_points(ctx, d_beta, t->betaTauG1, n))))
    return rc;
  const u256 *coefA = d_sum.get(), *coefB = d_sum.get() + n;
  if (run[G16_REL_A1]) {
    if ((rc = staged_msm<G1>(ctx, z_all, G16_SCALARS_STD, d->pointsA1, nv, &pb->lhs1[0]))) return rc;
    if ((rc = msm_device<G1>(ctx, coefA, G16_SCALARS_MONT, d_tau1.get(), n, &pb->rhs1[0], nullptr, 0))) return rc;
  }
  if (run[G16_REL_B1]) {
    if ((rc = staged_msm<G1>(ctx, z_all, G16_SCALARS_STD, d->pointsB1, nv, &pb->lhs1[1]))) return rc;
    if ((rc = msm_device<G1>(ctx, coefB, G16_SCALARS_MONT, d_tau1.get(), n, &pb->rhs1[1], nullptr, 0))) return rc;
  }
  if (run[G16_REL_B2]) {
    if ((rc = staged_msm<G2>(ctx, z_all, G16_SCALARS_STD, d->pointsB2, nv, &pb->lhs2))) return rc;
    if ((rc = msm_device<G2>(ctx, coefB, G16_SCALARS_MONT, d_tau2.get(), n, &pb->rhs2, nullptr, 0))) return rc;
  }
  for (int j = 0; j < 2; ++j) {
    if (!pair4[j]) continue;
    const int h = j == 0 ? 1 : 0;   // the half of the product buffers: 0 = pub, 1 = priv
    const u256 *cA = d_ab.get() + 3 * n * h, *cB = cA + n, *cC = d_cc.get() + 3 * n * h;
    if (j == 0)
      rc = staged_msm<G1>(ctx, z_priv + npubs + 1, G16_SCALARS_STD, d->pointsC1, npriv, pt.d_P(0, 0));
    else
      rc = staged_msm<G1>(ctx, z_pub, G16_SCALARS_STD, vk->pointsIC, (size_t)npubs + 1, pt.d_P(1, 0));
    if (rc) return rc;
    if ((rc = msm_device<G1>(ctx, cA, G16_SCALARS_MONT, d_beta.get(), n, pt.d_P(j, 1), nullptr, 0))) return rc;
    if ((rc = msm_device<G1>(ctx, cB, G16_SCALARS_MONT, d_alpha.get(), n, pt.d_P(j, 2), nullptr, 0))) return rc;
    if ((rc = msm_device<G1>(ctx, cC, G16_SCALARS_MONT, d_tau1.get(), n, pt.d_P(j, 3), nullptr, 0))) return rc;
  }
  if (run[G16_REL_H1]) {
    if ((rc = staged_msm<G1>(ctx, d_ystd.get(), G16_SCALARS_STD, d->pointsH1, n, pt.d_P(2, 0)))) return rc;
    if ((rc = msm_device<G1>(ctx, d_h.get(), G16_SCALARS_MONT, d_tau1.get(), 2 * n, pt.d_P(2, 1), nullptr, 0))) return rc;
  }
  // 8. the pairing products, e(-L, delta2 / gamma2) * prod e(R_k, gen2) == 1, as ONE launch of three workgroups: each is
  //    the latency of one lane's Miller loop and final exponentiation, so side by side they cost what one does.
  if ((pair4[0] || pair4[1] || run[G16_REL_H1]) && (rc = pt.run(ctx, 1u))) return rc;
  SumBuf got;
  HIPCHK(ctx, hipMemcpyAsync(&got, pb, sizeof got, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));

  // 9. the verdicts
  if (run[G16_REL_COEFFS_A])
    for (int k = 0; k < 2; ++k) {
      rel[G16_REL_COEFFS_A + k] = first[k] == 0xffffffffu;
      out->first_row[k] = first[k] == 0xffffffffu ? NONE : (size_t)first[k];
    }
  if (run[G16_REL_A1]) rel[G16_REL_A1] = !memcmp(&got.lhs1[0], &got.rhs1[0], sizeof(g1_aff));
  if (run[G16_REL_B1]) rel[G16_REL_B1] = !memcmp(&got.lhs1[1], &got.rhs1[1], sizeof(g1_aff));
  if (run[G16_REL_B2]) rel[G16_REL_B2] = !memcmp(&got.lhs2, &got.rhs2, sizeof(g2_aff));
  if (run[G16_REL_C1]) rel[G16_REL_C1] = npriv ? pt.result(0) : 1;
  if (run[G16_REL_IC]) rel[G16_REL_IC] = pt.result(1);
  if (run[G16_REL_H1]) rel[G16_REL_H1] = pt.result(2);
  fold_report(CIRCUIT_RELATIONS, run, nullptr, 0, rel, nullptr, out->failed);
  return G16_OK;
}

}  // namespace

extern "C" int32_t g16_circuit_audit(g16_ctx* ctx, const g16_pkey_desc* desc, const g16_vkey_desc* vk,
                                     const void* section4, size_t section4_bytes, const g16_r1cs_desc* r1cs,
                                     const g16_ptau_desc* ptau, const void* wire_multipliers, const void* h_multipliers,
                                     g16_circuit_report* out) {
  if (!ctx) return G16_EINVAL;
  int32_t rc;
  if ((rc = validate(ctx, desc, r1cs, ptau, wire_multipliers, h_multipliers, out))) return rc;
  {   // a zero multiplier: the index goes to the error text (the widened copies are made on the device later)
    std::vector<uint64_t> tmp;
    if ((rc = g16_widen_multipliers(ctx, "g16_circuit_audit: wire", wire_multipliers, desc->nvars, tmp))) return rc;
    if ((rc = g16_widen_multipliers(ctx, "g16_circuit_audit: h", h_multipliers, size_t(1) << desc->log2_domain, tmp)))
      return rc;
  }
  memset(out, 0, sizeof *out);
  for (int k = 0; k < G16_CIRCUIT_RELATIONS; ++k) out->relation[k] = -1;
  out->first_row[0] = out->first_row[1] = NONE;
  // the key's own audit first: it checks the description before it queues anything, and waits for its work
  if ((rc = g16_key_audit_body(ctx, desc, vk, section4, section4_bytes, wire_multipliers, &out->key))) return rc;
  if (out->key.failed) out->failed |= G16_CIRCUIT_KEY;
  CTX_ENTER(ctx);
  return no_throw(   // the matrices are arranged in host vectors
      ctx, [&] { return circuit_audit(ctx, desc, vk, section4, r1cs, ptau, wire_multipliers, h_multipliers, out); },
      "out of host memory while arranging the matrices");
}
