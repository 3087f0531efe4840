// Circuit setup (include/g16hip.h, "circuit setup"): the proving key of `snarkjs zkey new` from an R1CS and the powers
// of tau of a ceremony, with no toxic waste in sight.  The Lagrange form of the powers is an inverse NTT whose elements
// are curve points; every point array of the key is a sparse matrix applied to such a vector.  Host layer of
// g16_points_intt_g1/g2 and g16_circuit_setup; kernels: circuit_setup.cuh, launch shapes: circuit_setup_plan.hpp.  The
// element checks of the ptau are the circuit audit's (g16_audit_sections, audit.hip), the twiddles and coset factors
// come from the geometric-sequence kernel of the fake setup (setup.hip).
#include "checker.hpp"
#include "setup.cuh"

using namespace g16;

namespace {

u256 std_u32(uint32_t x) {
  u256 o = Fr::zero();
  o.v[0] = x;
  return o;
}
// 1 / 2^k, Montgomery
u256 inv_pow2(uint32_t k) {
  u256 x = Fr::one();
  for (uint32_t i = 0; i < k; ++i) x = Fr::div2(x);
  return x;
}

// tw[k] = omega^-k of the 2^log2n domain in standard form, k < 2^(log2n-1): a Montgomery sequence times the integer 1
int32_t make_twiddles(g16_ctx* ctx, uint32_t log2n, u256* d_tw) {
  return g16_setup_geometric(ctx, false, Fr::one(), Fr::inv(setup_omega(log2n)), std_u32(1), Fr::zero(),
                             pintt_twiddles(log2n), d_tw, nullptr);
}

// d_out[k] = sum_j (omega^-jk) d_scal[vstride j] d_in[j]: load in bit-reversed order with the scalars applied (1/n, one
// for all, or a factor per element), the stages in place, then affine.  d_work: 2^log2n XYZZ points.
template <class C>
int32_t points_intt_device(g16_ctx* ctx, const void* d_in, const u256* d_scal, uint32_t vstride, uint32_t log2n,
                           const u256* d_tw, void* d_work, void* d_out) {
  const size_t n = size_t(1) << log2n;
  int32_t rc;
  if ((rc = cs_term_device<C>(ctx, d_in, nullptr, d_scal, nullptr, vstride, 0, log2n, n, d_work))) return rc;
  if ((rc = cs_butterflies_device<C>(ctx, d_work, d_tw, log2n))) return rc;
  return cs_to_affine_device<C>(ctx, d_work, n, d_out);
}

template <class C>
int32_t points_intt(g16_ctx* ctx, const void* points, uint32_t log2n, void* out) {
  if (!ctx) return G16_EINVAL;
  if (!points || !out) {
    ctx->err = "g16_points_intt: null pointer argument";
    return G16_EINVAL;
  }
  if (log2n > PINTT_MAX_LOG2) {
    ctx->err = "g16_points_intt: log2n out of range (must be <= 24)";
    return G16_EINVAL;
  }
  CTX_ENTER(ctx);
  const size_t n = size_t(1) << log2n;
  const u256 inv_n = Fr::from_mont(inv_pow2(log2n));   // lives until the wait below
  DevMem<typename C::Aff> d_pts;
  DevMem<typename C::Acc> d_work;
  DevMem<u256> d_tw;
  SyncOnExit drain{ctx->stream};
  HIPCHK(ctx, dev_alloc(d_pts, n * sizeof(typename C::Aff)));
  HIPCHK(ctx, dev_alloc(d_work, n * sizeof(typename C::Acc)));
  HIPCHK(ctx, dev_alloc(d_tw, (pintt_twiddles(log2n) + 1) * 32));
  HIPCHK(ctx, hipMemcpyAsync(d_pts.get(), points, n * sizeof(typename C::Aff), hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(d_tw.get() + pintt_twiddles(log2n), &inv_n, 32, hipMemcpyHostToDevice, ctx->stream));
  int32_t rc;
  if ((rc = make_twiddles(ctx, log2n, d_tw.get()))) return rc;
  if ((rc = points_intt_device<C>(ctx, d_pts.get(), d_tw.get() + pintt_twiddles(log2n), 0, log2n, d_tw.get(),
                                  d_work.get(), d_pts.get())))
    return rc;
  HIPCHK(ctx, hipMemcpyAsync(out, d_pts.get(), n * sizeof(typename C::Aff), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return G16_OK;
}

// a 32-byte scalar of the caller: canonical (< r), to Montgomery form if it came in standard form
bool load_scalar(const void* p, bool mont, u256& out) {
  u256 v;
  memcpy(&v, p, 32);
  if (!Fr::is_canonical(v)) return false;
  out = mont ? v : Fr::to_mont(v);
  return true;
}

// everything g16_circuit_setup rejects before it queues anything; delta comes back in Montgomery form (one: NULL)
int32_t validate(g16_ctx* ctx, const g16_r1cs_desc* r, const g16_ptau_desc* t, const void* delta,
                 const g16_setup_points* o, uint32_t& log2_dom, u256& delta_mont) {
  static const char who[] = "g16_circuit_setup";
  if (!r || !t || !o) return fail(ctx, who, "null argument");
  if (!t->tauG1 || !t->tauG2 || !t->alphaTauG1 || !t->betaTauG1 || !t->betaG2) return fail(ctx, who, "null ptau section");
  for (int k = 0; k < 3; ++k)
    if (r->nnz[k] && (!r->row[k] || !r->col[k] || !r->val[k])) return fail(ctx, who, "null matrix pointer");
  if (r->flavour != G16_FLAVOUR_JENSGROTH && r->flavour != G16_FLAVOUR_SNARKJS) return fail(ctx, who, "unknown flavour");
  if (r->flags != G16_SCALARS_MONT && r->flags != G16_SCALARS_STD)
    return fail(ctx, who, "r1cs flags must be G16_SCALARS_MONT or _STD");
  if (r->nvars <= r->npubs) return fail(ctx, who, "nvars must exceed npubs (wire 0 is the constant one)");
  if (!o->alpha1 || !o->beta1 || !o->delta1 || !o->beta2 || !o->gamma2 || !o->delta2 || !o->pointsIC || !o->pointsA1 ||
      !o->pointsB1 || !o->pointsB2 || !o->pointsH1 || (r->nvars > r->npubs + 1 && !o->pointsC1))
    return fail(ctx, who, "null output pointer");
  log2_dom = setup_log2_domain(r->nconstraints, r->npubs);
  if (log2_dom > PINTT_MAX_LOG2) return fail(ctx, who, "domain too large (must not exceed 2^24)");
  if (t->power < log2_dom + 1 || t->power > 28)
    return fail(ctx, who, "the powers of tau are too short: power >= log2_domain + 1 is needed (tau^(2n-1); and power <= 28)");
  if ((uint64_t)r->nnz[0] + r->nnz[1] + r->nnz[2] + r->npubs + 1 >= 0xffffffffu)
    return fail(ctx, who, "too many matrix entries");
  delta_mont = Fr::one();
  if (delta && !load_scalar(delta, r->flags == G16_SCALARS_MONT, delta_mont))
    return fail(ctx, who, "delta is not canonical (>= r)");
  if (Fr::is_zero(delta_mont)) return fail(ctx, who, "delta must not be zero");
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

// One sparse product: entries (wire, source point, value index) sorted by wire, and the sum pass's wires by bin.
// The host vectors live as long as the device copies are in flight.
struct MatrixPart {
  const uint32_t *wire, *row;   // both null: the dummy entries (wire i, row first_row + i)
  size_t count;
  uint32_t first_row;           // added to the row: the dummy rows' start, or the point vector's offset
  uint32_t first_ord;           // index of the part's first value in the device value array
};
struct SparseJob {
  std::vector<uint32_t> idx;    // src | ord | off (nwires + 1) | wires (nwires)
  size_t count = 0;
  uint32_t nwires = 0;
  CsSumPlan plan{};
  DevMem<uint32_t> d_idx;
  const uint32_t* d_src() const { return d_idx.get(); }
  const uint32_t* d_ord() const { return d_idx.get() + count; }
  const uint32_t* d_off() const { return d_idx.get() + 2 * count; }
  const uint32_t* d_wires() const { return d_idx.get() + 2 * count + nwires + 1; }
};
int32_t job_build(g16_ctx* ctx, SparseJob& j, uint32_t nwires, const MatrixPart* parts, int nparts) {
  j.count = 0, j.nwires = nwires;
  for (int p = 0; p < nparts; ++p) j.count += parts[p].count;
  j.idx.assign(2 * j.count + 2 * (size_t)nwires + 1, 0);
  uint32_t *src = j.idx.data(), *ord = src + j.count, *off = ord + j.count, *wires = off + nwires + 1;
  std::vector<uint32_t> len(nwires, 0);
  for (int p = 0; p < nparts; ++p)
    for (size_t i = 0; i < parts[p].count; ++i) ++len[parts[p].wire ? parts[p].wire[i] : (uint32_t)i];
  for (uint32_t w = 0; w < nwires; ++w) off[w + 1] = off[w] + len[w];
  std::vector<uint32_t> cursor(off, off + nwires);
  for (int p = 0; p < nparts; ++p)
    for (size_t i = 0; i < parts[p].count; ++i) {
      const uint32_t at = cursor[parts[p].wire ? parts[p].wire[i] : (uint32_t)i]++;
      src[at] = parts[p].first_row + (parts[p].row ? parts[p].row[i] : (uint32_t)i);
      ord[at] = parts[p].first_ord + (uint32_t)i;
    }
  j.plan = cs_sum_plan(len.data(), nwires, wires);
  HIPCHK(ctx, dev_alloc(j.d_idx, j.idx.size() * 4));
  HIPCHK(ctx, hipMemcpyAsync(j.d_idx.get(), j.idx.data(), j.idx.size() * 4, hipMemcpyHostToDevice, ctx->stream));
  return G16_OK;
}
// d_out[w] = sum over the entries of wire w of value * d_pts[source], affine; d_terms: j.count XYZZ points
template <class C>
int32_t job_run(g16_ctx* ctx, const SparseJob& j, const void* d_pts, const u256* d_val, uint32_t mont, void* d_terms,
                void* d_out) {
  if (int32_t rc = cs_term_device<C>(ctx, d_pts, j.d_src(), d_val, j.d_ord(), 1, mont, 0, j.count, d_terms)) return rc;
  return cs_segsum_device<C>(ctx, d_terms, j.d_off(), j.d_wires(), j.plan, d_out);
}

int32_t circuit_setup(g16_ctx* ctx, const g16_r1cs_desc* r, const g16_ptau_desc* t, bool with_delta, const u256& delta,
                      uint32_t L, g16_setup_points* o) {
  const uint32_t nv = r->nvars, npubs = r->npubs, ncons = r->nconstraints, np1 = npubs + 1;
  const size_t n = size_t(1) << L, npriv = (size_t)nv - np1;
  const bool snarkjs = r->flavour == G16_FLAVOUR_SNARKJS;
  const uint32_t mont = r->flags == G16_SCALARS_MONT ? 1u : 0u;
  int32_t rc;

  // 1. the audit's element passes over what is read of the five ptau arrays
  {
    const g16_audit_section psec[G16_PTAU_SECTIONS] = {
        {1, t->tauG1, 2 * n}, {2, t->tauG2, n}, {1, t->alphaTauG1, n}, {1, t->betaTauG1, n}, {2, t->betaG2, 1}};
    ElementPass pass;
    if ((rc = pass.run(ctx, CIRCUIT_SETUP_ARRAYS, psec)) || (rc = pass.first_finding(ctx, "g16_circuit_setup"))) return rc;
  }

  // 2. the scalars every stage shares, in device memory: standard form unless noted
  enum { K_INV_N = 0, K_DELTA, K_DELTA_INV, K_COUNT };
  const u256 delta_inv = Fr::inv(delta);
  const u256 consts[K_COUNT] = {Fr::from_mont(inv_pow2(L)), Fr::from_mont(delta), Fr::from_mont(delta_inv)};
  g1_aff gen1 = host_gen1();
  g2_aff gen2 = host_gen2();
  const size_t nnzA = r->nnz[0], nnzB = r->nnz[1], nnzC = r->nnz[2], nval = nnzA + np1 + nnzB + nnzC;
  std::vector<u256> ones(np1, mont ? Fr::one() : std_u32(1));   // the dummy entries' values, in the form of the others

  // owners first, the drain of the stream that uses them last (released in reverse order)
  SparseJob jobA, jobB, jobComb;
  DevMem<u256> d_consts, d_tw, d_hscal, d_val;
  DevMem<g1_aff> d_tau1, d_alpha, d_beta, d_lag1, d_hx, d_h1, d_a1, d_b1, d_comb, d_c1, d_spec1;
  DevMem<g2_aff> d_tau2, d_lag2, d_b2, d_spec2;
  DevMem<> d_work;
  SyncOnExit drain{ctx->stream};
  auto up = [&](void* dst, const void* src, size_t bytes) {
    return bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, ctx->stream) : hipSuccess;
  };
  HIPCHK(ctx, dev_alloc(d_consts, sizeof consts));
  HIPCHK(ctx, up(d_consts.get(), consts, sizeof consts));
  HIPCHK(ctx, dev_alloc(d_tw, (pintt_twiddles(L) + 1) * 32));
  if ((rc = make_twiddles(ctx, L, d_tw.get()))) return rc;
  HIPCHK(ctx, dev_alloc(d_tau1, 2 * n * sizeof(g1_aff)));
  HIPCHK(ctx, dev_alloc(d_tau2, n * sizeof(g2_aff)));
  HIPCHK(ctx, dev_alloc(d_alpha, n * sizeof(g1_aff)));
  HIPCHK(ctx, dev_alloc(d_beta, n * sizeof(g1_aff)));
  HIPCHK(ctx, up(d_tau1.get(), t->tauG1, 2 * n * sizeof(g1_aff)));
  HIPCHK(ctx, up(d_tau2.get(), t->tauG2, n * sizeof(g2_aff)));
  HIPCHK(ctx, up(d_alpha.get(), t->alphaTauG1, n * sizeof(g1_aff)));
  HIPCHK(ctx, up(d_beta.get(), t->betaTauG1, n * sizeof(g1_aff)));

  // 3. the entry lists: A (with the dummy entries) and B by wire; comb = A over LbG1, B over LaG1, C over LG1 as ONE
  //    list over the vector LG1 | LaG1 | LbG1.  Values: A | ones | B | C.
  const uint32_t ordB = (uint32_t)(nnzA + np1), ordC = (uint32_t)(ordB + nnzB);
  const MatrixPart pa[2] = {{r->col[0], r->row[0], nnzA, 0, 0}, {nullptr, nullptr, np1, ncons, (uint32_t)nnzA}};
  const MatrixPart pb[1] = {{r->col[1], r->row[1], nnzB, 0, ordB}};
  const MatrixPart pc[4] = {{r->col[0], r->row[0], nnzA, (uint32_t)(2 * n), 0},
                            {nullptr, nullptr, np1, (uint32_t)(2 * n) + ncons, (uint32_t)nnzA},
                            {r->col[1], r->row[1], nnzB, (uint32_t)n, ordB},
                            {r->col[2], r->row[2], nnzC, 0, ordC}};
  if ((rc = job_build(ctx, jobA, nv, pa, 2)) || (rc = job_build(ctx, jobB, nv, pb, 1)) ||
      (rc = job_build(ctx, jobComb, nv, pc, 4)))
    return rc;
  HIPCHK(ctx, dev_alloc(d_val, nval * 32));
  HIPCHK(ctx, up(d_val.get(), r->val[0], nnzA * 32));
  HIPCHK(ctx, up(d_val.get() + nnzA, ones.data(), (size_t)np1 * 32));
  HIPCHK(ctx, up(d_val.get() + ordB, r->val[1], nnzB * 32));
  HIPCHK(ctx, up(d_val.get() + ordC, r->val[2], nnzC * 32));
  // one work area: the working vector of a transform, then the terms of one matrix at a time
  size_t work = n * sizeof(g2_acc);
  if (jobComb.count * sizeof(g1_acc) > work) work = jobComb.count * sizeof(g1_acc);
  if (jobB.count * sizeof(g2_acc) > work) work = jobB.count * sizeof(g2_acc);
  if ((size_t)nv * sizeof(g1_acc) > work) work = (size_t)nv * sizeof(g1_acc);
  HIPCHK(ctx, dev_alloc(d_work, work));
  HIPCHK(ctx, dev_alloc(d_lag1, 3 * n * sizeof(g1_aff)));
  HIPCHK(ctx, dev_alloc(d_lag2, n * sizeof(g2_aff)));
  HIPCHK(ctx, dev_alloc(d_hx, n * sizeof(g1_aff)));
  HIPCHK(ctx, dev_alloc(d_h1, n * sizeof(g1_aff)));
  HIPCHK(ctx, dev_alloc(d_hscal, n * 32));
  HIPCHK(ctx, dev_alloc(d_a1, (size_t)nv * sizeof(g1_aff)));
  HIPCHK(ctx, dev_alloc(d_b1, (size_t)nv * sizeof(g1_aff)));
  HIPCHK(ctx, dev_alloc(d_b2, (size_t)nv * sizeof(g2_aff)));
  HIPCHK(ctx, dev_alloc(d_comb, (size_t)nv * sizeof(g1_aff)));
  HIPCHK(ctx, dev_alloc(d_c1, (npriv ? npriv : 1) * sizeof(g1_aff)));
  HIPCHK(ctx, dev_alloc(d_spec1, 2 * sizeof(g1_aff)));
  HIPCHK(ctx, dev_alloc(d_spec2, 2 * sizeof(g2_aff)));

  // 4. the Lagrange forms: LG1 | LaG1 | LbG1 and LG2
  const u256 *k_inv_n = d_consts.get() + K_INV_N, *k_delta = d_consts.get() + K_DELTA,
             *k_delta_inv = d_consts.get() + K_DELTA_INV;
  const g1_aff* srcs[3] = {d_tau1.get(), d_alpha.get(), d_beta.get()};
  for (int k = 0; k < 3; ++k)
    if ((rc = points_intt_device<G1>(ctx, srcs[k], k_inv_n, 0, L, d_tw.get(), d_work.get(), d_lag1.get() + k * n)))
      return rc;
  if ((rc = points_intt_device<G2>(ctx, d_tau2.get(), k_inv_n, 0, L, d_tw.get(), d_work.get(), d_lag2.get()))) return rc;

  // 5. pointsH1
  const g1_aff* h_out = d_h1.get();
  if (snarkjs) {
    // delta^-1 L'_(2i+1)(tau) gen1 on the doubled domain = the size-n transform of (tauG1[j] - tauG1[j+n]) eta^-j / 2,
    // eta = omega_2n: element j is loaded with the factor delta^-1 eta^-j / (2n)
    if ((rc = cs_diff_device<G1>(ctx, d_tau1.get(), d_tau1.get() + n, n, d_hx.get()))) return rc;
    const u256 c = Fr::from_mont(Fr::mul(delta_inv, inv_pow2(L + 1)));
    if ((rc = g16_setup_geometric(ctx, false, Fr::one(), Fr::inv(setup_omega(L + 1)), c, Fr::zero(), n, d_hscal.get(),
                                  nullptr)))
      return rc;
    if ((rc = points_intt_device<G1>(ctx, d_hx.get(), d_hscal.get(), 1, L, d_tw.get(), d_work.get(), d_h1.get())))
      return rc;
  } else {
    // delta^-1 (tauG1[i+n] - tauG1[i])
    if ((rc = cs_diff_device<G1>(ctx, d_tau1.get() + n, d_tau1.get(), n, d_hx.get()))) return rc;
    if (with_delta) {
      if ((rc = cs_term_device<G1>(ctx, d_hx.get(), nullptr, k_delta_inv, nullptr, 0, 0, 0, n, d_work.get()))) return rc;
      if ((rc = cs_to_affine_device<G1>(ctx, d_work.get(), n, d_h1.get()))) return rc;
    } else {
      h_out = d_hx.get();
    }
  }

  // 6. the sparse products, one matrix after the other through the one term buffer
  if ((rc = job_run<G1>(ctx, jobA, d_lag1.get(), d_val.get(), mont, d_work.get(), d_a1.get()))) return rc;
  if ((rc = job_run<G1>(ctx, jobB, d_lag1.get(), d_val.get(), mont, d_work.get(), d_b1.get()))) return rc;
  if ((rc = job_run<G2>(ctx, jobB, d_lag2.get(), d_val.get(), mont, d_work.get(), d_b2.get()))) return rc;
  if ((rc = job_run<G1>(ctx, jobComb, d_lag1.get(), d_val.get(), mont, d_work.get(), d_comb.get()))) return rc;
  const g1_aff* c_out = d_comb.get() + np1;
  if (with_delta && npriv) {
    if ((rc = cs_term_device<G1>(ctx, d_comb.get() + np1, nullptr, k_delta_inv, nullptr, 0, 0, 0, npriv, d_work.get())))
      return rc;
    if ((rc = cs_to_affine_device<G1>(ctx, d_work.get(), npriv, d_c1.get()))) return rc;
    c_out = d_c1.get();
  }

  // 7. delta1, delta2
  HIPCHK(ctx, up(d_spec1.get(), &gen1, sizeof gen1));
  HIPCHK(ctx, up(d_spec2.get(), &gen2, sizeof gen2));
  const g1_aff* delta1 = d_spec1.get();
  const g2_aff* delta2 = d_spec2.get();
  if (with_delta) {
    if ((rc = cs_term_device<G1>(ctx, d_spec1.get(), nullptr, k_delta, nullptr, 0, 0, 0, 1, d_work.get()))) return rc;
    if ((rc = cs_to_affine_device<G1>(ctx, d_work.get(), 1, d_spec1.get() + 1))) return rc;
    if ((rc = cs_term_device<G2>(ctx, d_spec2.get(), nullptr, k_delta, nullptr, 0, 0, 0, 1, d_work.get()))) return rc;
    if ((rc = cs_to_affine_device<G2>(ctx, d_work.get(), 1, d_spec2.get() + 1))) return rc;
    delta1 = d_spec1.get() + 1, delta2 = d_spec2.get() + 1;
  }

  // 8. the points to the caller
  auto down = [&](void* dst, const void* src, size_t bytes) {
    return bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream) : hipSuccess;
  };
  HIPCHK(ctx, down(o->pointsA1, d_a1.get(), (size_t)nv * sizeof(g1_aff)));
  HIPCHK(ctx, down(o->pointsB1, d_b1.get(), (size_t)nv * sizeof(g1_aff)));
  HIPCHK(ctx, down(o->pointsB2, d_b2.get(), (size_t)nv * sizeof(g2_aff)));
  HIPCHK(ctx, down(o->pointsIC, d_comb.get(), (size_t)np1 * sizeof(g1_aff)));
  HIPCHK(ctx, down(o->pointsC1, c_out, npriv * sizeof(g1_aff)));
  HIPCHK(ctx, down(o->pointsH1, h_out, n * sizeof(g1_aff)));
  HIPCHK(ctx, down(o->delta1, delta1, sizeof(g1_aff)));
  HIPCHK(ctx, down(o->delta2, delta2, sizeof(g2_aff)));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  memcpy(o->alpha1, t->alphaTauG1, sizeof(g1_aff));
  memcpy(o->beta1, t->betaTauG1, sizeof(g1_aff));
  memcpy(o->beta2, t->betaG2, sizeof(g2_aff));
  memcpy(o->gamma2, &gen2, sizeof(g2_aff));
  return G16_OK;
}

}  // namespace

extern "C" int32_t g16_points_intt_g1(g16_ctx* ctx, const void* points, uint32_t log2n, void* out) {
  return points_intt<G1>(ctx, points, log2n, out);
}
extern "C" int32_t g16_points_intt_g2(g16_ctx* ctx, const void* points, uint32_t log2n, void* out) {
  return points_intt<G2>(ctx, points, log2n, out);
}

extern "C" int32_t g16_circuit_setup(g16_ctx* ctx, const g16_r1cs_desc* r1cs, const g16_ptau_desc* ptau,
                                     const void* delta, g16_setup_points* out) {
  if (!ctx) return G16_EINVAL;
  uint32_t log2_dom = 0;
  u256 delta_mont;
  if (int32_t rc = validate(ctx, r1cs, ptau, delta, out, log2_dom, delta_mont)) return rc;
  CTX_ENTER(ctx);
  return no_throw(   // the entry lists are sorted in host vectors
      ctx, [&] { return circuit_setup(ctx, r1cs, ptau, delta != nullptr, delta_mont, log2_dom, out); },
      "out of host memory while arranging the matrices");
}
