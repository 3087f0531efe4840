// The shape of a checker, the part that touches HIP: what the key audit, the circuit audit, the two ceremony
// verifiers and the two contribute calls do alike.  What they decide is relation_plan.hpp; this is what they queue from
// it: the element passes over a table of arrays (ElementPass), the rows of pairing products (ProductTable) and the MSM
// over a host point array (staged_msm).  Host code only: every kernel stays in the unit that launched it before.
#pragma once
#include <new>

#include "g16_internal.hpp"
#include "ec.cuh"
#include "relation_plan.hpp"

void g16_curve_consts_g2(void* gen2, void* twist_b);   // msm_g2_misc.hip: gen2 (128 B), twistCoeffB (64 B)

namespace g16 {

inline g1_aff host_gen1() { return g1_aff{Fp::one(), Fp::dbl(Fp::one())}; }   // (1, 2), curves.nim:112-113
inline g2_aff host_gen2() {
  g2_aff gen2;
  fp2_t twist_b;
  g16_curve_consts_g2(&gen2, &twist_b);
  return gen2;
}

// ---- entry helpers -----------------------------------------------------------------------------------------------------------
// G16_EINVAL with "<who>: <msg>" as the context's error text
inline int32_t fail(g16_ctx* ctx, const char* who, const std::string& msg) {
  ctx->err = std::string(who) + ": " + msg;
  return G16_EINVAL;
}
// fn() for a body that fills host vectors or builds strings: no exception may cross the C ABI
template <class Fn>
inline int32_t no_throw(g16_ctx* ctx, Fn&& fn, const char* text = "out of host memory") {
  try {
    return fn();
  } catch (const std::bad_alloc&) {
    ctx->err = text;
    return G16_ENOMEM;
  }
}
// a 32-byte scalar of the caller, canonical and non-zero, to Montgomery form
inline bool load_scalar_nonzero_mont(const void* p, bool mont, u256& mont_out) {
  u256 v;
  memcpy(&v, p, 32);
  if (!Fr::is_canonical(v) || Fr::is_zero(v)) return false;
  mont_out = mont ? v : Fr::to_mont(v);
  return true;
}

// ---- the element passes over a table of arrays, then the scan for (0,0) --------------------------------------------------
struct ElementPass {
  enum { MAX = G16_PTAU_REPORT_ARRAYS };
  const ArrayTable* t = nullptr;
  int rows = 0;                       // t->n, and one more for the coefficient pass
  size_t first_bad[MAX][3], bad_count[MAX][3], first_infinity[MAX];
  uint32_t dirty = 0, infinite = 0;   // bit a: array a has an element that fails a check / that is (0,0)

  // `sec`: the t->n arrays; `coeffs` (the key audit): one more pass in the same counts buffer.  One wait, at the end.
  int32_t run(g16_ctx* ctx, const ArrayTable& table, const g16_audit_section* sec, const g16_audit_coeffs* coeffs = nullptr) {
    t = &table, rows = table.n + (coeffs ? 1 : 0);
    if (int32_t rc = g16_audit_sections(ctx, sec, table.n, first_bad, bad_count, coeffs)) return rc;
    dirty = dirty_mask(bad_count, rows);
    for (int a = 0; a < table.n; ++a) {
      first_infinity[a] = NONE;
      const size_t psz = sec[a].group == 1 ? sizeof(g1_aff) : sizeof(g2_aff);
      for (size_t i = 0; a < table.nscan && i < sec[a].n; ++i)
        if (is_infinity((const char*)sec[a].p + psz * i, psz)) {
          first_infinity[a] = i, infinite |= 1u << a;
          break;
        }
    }
    return G16_OK;
  }
  uint32_t clean() const { return ~(dirty | infinite); }   // bit a: the relations may read array a
  bool all_clean() const { return !(dirty | infinite); }

  // sink 1 (the contribute calls, the circuit setup): the first finding as the error text of `who`
  int32_t first_finding(g16_ctx* ctx, const char* who) const {
    for (int a = 0; a < t->n; ++a)
      for (int k = 0; k < 3; ++k)
        if (bad_count[a][k]) return fail(ctx, who, finding_text(t->row[a].name, first_bad[a][k], k, bad_count[a][k]));
    for (int a = 0; a < t->n; ++a)
      if (first_infinity[a] != NONE) return fail(ctx, who, infinity_text(t->row[a].name, first_infinity[a]));
    return G16_OK;
  }
  // sink 2 (the audits, the verifiers): into a report
  void to_report(size_t (*out_first_bad)[3], size_t (*out_bad_count)[3], size_t* out_first_infinity = nullptr) const {
    memcpy(out_first_bad, first_bad, rows * sizeof first_bad[0]);
    memcpy(out_bad_count, bad_count, rows * sizeof bad_count[0]);
    if (out_first_infinity) memcpy(out_first_infinity, first_infinity, t->n * sizeof(size_t));
  }
};

// ---- MSMs over host arrays, through the context's staging buffers ---------------------------------------------------------
// n standard-form scalars of the host into stage_s
inline int32_t stage_scalars(g16_ctx* ctx, const uint64_t* scalars, size_t n) {
  if (!n) return G16_OK;
  if (int32_t rc = ensure(ctx, ctx->stage_s, n * 32)) return rc;
  HIPCHK(ctx, hipMemcpyAsync(ctx->stage_s.p(), scalars, n * 32, hipMemcpyHostToDevice, ctx->stream));
  return G16_OK;
}
// n points of the host into stage_p
template <class C>
inline int32_t stage_points(g16_ctx* ctx, const void* host_points, size_t n) {
  constexpr size_t psz = sizeof(typename C::Aff);
  if (int32_t rc = ensure(ctx, ctx->stage_p, n * psz)) return rc;
  HIPCHK(ctx, hipMemcpyAsync(ctx->stage_p.p(), host_points, n * psz, hipMemcpyHostToDevice, ctx->stream));
  return G16_OK;
}
// d_out[off] = sum_{i < n} s_i P_{i + off}, off < shifts, for a HOST point array of n + shifts - 1 points (one upload) and
// device scalars (stage_s after stage_scalars, or the caller's own).  n == 0: the slots keep what they hold, (0,0).
template <class C>
inline int32_t staged_msm(g16_ctx* ctx, const void* d_scalars, uint32_t flags, const void* host_points, size_t n, void* d_out,
                          int shifts = 1) {
  if (!n) return G16_OK;
  if (int32_t rc = stage_points<C>(ctx, host_points, n + shifts - 1)) return rc;
  for (int off = 0; off < shifts; ++off)
    if (int32_t rc = msm_device<C>(ctx, d_scalars, flags, (const typename C::Aff*)ctx->stage_p.p() + off, n,
                                   (typename C::Aff*)d_out + off, nullptr, 0))
      return rc;
  return G16_OK;
}

// ---- rows of four pairs (P, Q), one pairing product per row: result(row) = ( prod_k e(+-P_k, Q_k) == 1 ) ------------------
// A pair that is never set, and so every row that is not run, keeps (0,0) on both sides and contributes one.  The caller
// declares its SyncOnExit after the table, sets the pairs the host knows, uploads, lets sums land in d_P / d_Q, runs and,
// after its wait, reads result().
struct ProductTable {
  std::vector<g1_aff> P;
  std::vector<g2_aff> Q;
  std::vector<int32_t> res;
  DevMem<g1_aff> d_p;
  DevMem<g2_aff> d_q;
  DevMem<int32_t> d_res;

  explicit ProductTable(size_t rows) : P(4 * rows), Q(4 * rows), res(rows, 0) {
    memset(P.data(), 0, P.size() * sizeof(g1_aff));
    memset(Q.data(), 0, Q.size() * sizeof(g2_aff));
  }
  void set(size_t row, int pair, const void* g1, const void* g2) {   // either may be null: a sum will land there
    if (g1) memcpy(&P[4 * row + pair], g1, sizeof(g1_aff));
    if (g2) memcpy(&Q[4 * row + pair], g2, sizeof(g2_aff));
  }
  int32_t upload(g16_ctx* ctx) {
    HIPCHK(ctx, dev_alloc(d_p, P.size() * sizeof(g1_aff)));
    HIPCHK(ctx, dev_alloc(d_q, Q.size() * sizeof(g2_aff)));
    HIPCHK(ctx, dev_alloc(d_res, res.size() * sizeof(int32_t)));
    HIPCHK(ctx, hipMemcpyAsync(d_p.get(), P.data(), P.size() * sizeof(g1_aff), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(d_q.get(), Q.data(), Q.size() * sizeof(g2_aff), hipMemcpyHostToDevice, ctx->stream));
    return G16_OK;
  }
  g1_aff* d_P(size_t row, int pair) { return d_p.get() + 4 * row + pair; }
  g2_aff* d_Q(size_t row, int pair) { return d_q.get() + 4 * row + pair; }
  // every row in one launch (bit k of neg_mask negates pair k), and the results on their way back
  int32_t run(g16_ctx* ctx, uint32_t neg_mask) {
    if (int32_t rc = g16_pairing_products4(ctx, d_p.get(), d_q.get(), (uint32_t)res.size(), neg_mask, d_res.get())) return rc;
    HIPCHK(ctx, hipMemcpyAsync(res.data(), d_res.get(), res.size() * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    return G16_OK;
  }
  int32_t result(size_t row) const { return res[row]; }
};

}  // namespace g16
