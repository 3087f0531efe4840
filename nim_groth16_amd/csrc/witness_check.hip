// Witness check (include/g16hip.h, "witness check"): which constraints of a circuit does an untrusted witness break?
//
// A g16_r1cs is the circuit's A, B and C as ONE row-balanced sparse matrix (spmv.hip) of virtual rows 3 i + k over the
// nconstraints rows of the circuit: no dummy entries, no padding to a domain.  A check queues four kernels on the
// context's stream and waits once:
//   witness_canonical  one lane per value: >= r is counted, the first index kept (the semantics of AuditCounts, audit.cuh);
//                      lane 0 compares witness[0] with the encoding of 1
//   witness_spmv       spmv_binned<3, DICT>: A z | B z | C z, nconstraints values each
//   witness_rows       one lane per constraint: one Montgomery product, compare, one bit; a wave writes its 64 bits as
//                      one bitmap word and adds their number to the count
//   witness_list       one workgroup walks the bitmap in order (witness_plan.hpp) and writes the 16 smallest indices and
//                      the three sums at the first of them, in standard form
// The host does not wait between them, so the product of a witness with a value >= r IS queued; witness_rows and
// witness_list read the canonical count first (stream order) and then neither read the sums nor report anything.
//
// The form of the sums (header comment of spmv.hip) and what the row check makes of it:
//   Montgomery witness                      a R, b R, c R    mul(a R, b R) = a b R        against c R
//   standard witness, value dictionary      a R, b R, c R    (the dictionary's second table: (v R^2) w / R)   the same
//   standard witness, plain values          a, b, c          mul(to_mont(a), b) = a b     against c
// The sums are fully reduced, so equality of residues is equality of limbs.
#include <new>

#include "g16_internal.hpp"
#include "ff.cuh"
#include "witness_plan.hpp"

using namespace g16;

static_assert(WITNESS_LIST == G16_WITNESS_LIST, "witness_plan.hpp is the list of another report");

namespace {

// what the kernels report; `first_noncanonical` and `list` start as 0xff bytes, the rest as zero
struct WitnessDev {
  uint32_t first_noncanonical;
  uint32_t list[WITNESS_LIST];
  uint32_t noncanonical_count, one_bad, bad_count;
  u256 az, bz, cz;
};
constexpr size_t WITNESS_DEV_ONES = offsetof(WitnessDev, noncanonical_count);

__global__ void __launch_bounds__(WITNESS_BLOCK) witness_canonical(const u256* __restrict__ w, uint32_t n, u256 one,
                                                                   WitnessDev* __restrict__ rep) {
  const uint32_t e = blockIdx.x * WITNESS_BLOCK + threadIdx.x;
  if (e >= n) return;
  const u256 v = w[e];
  if (e == 0 && !Fr::eq(v, one)) rep->one_bad = 1u;
  if (Fr::is_canonical(v)) return;
  atomicMin(&rep->first_noncanonical, e);
  atomicAdd(&rep->noncanonical_count, 1u);
}

// sums = A z | B z | C z, m each
__global__ void __launch_bounds__(WITNESS_BLOCK) witness_rows(const u256* __restrict__ sums, uint32_t m, uint32_t sums_mont,
                                                              unsigned long long* __restrict__ bitmap, WitnessDev* rep) {
  if (rep->noncanonical_count) return;   // uniform: the values are not residues, the sums mean nothing
  const uint32_t i = blockIdx.x * WITNESS_BLOCK + threadIdx.x;
  bool bad = false;
  if (i < m) {
    u256 a = sums[i];
    const u256 b = sums[(size_t)m + i], c = sums[2 * (size_t)m + i];
    if (!sums_mont) a = Fr::to_mont(a);
    bad = !Fr::eq(Fr::mul(a, b), c);
  }
  const unsigned long long mask = __ballot(bad);
  if ((threadIdx.x & 63) == 0 && i < m) {   // the wave's first constraint exists <=> its bitmap word does
    bitmap[i >> 6] = mask;
    if (mask) atomicAdd(&rep->bad_count, (uint32_t)__popcll(mask));
  }
}

// ONE workgroup: the walk of witness_plan.hpp
__global__ void __launch_bounds__(WITNESS_LANES) witness_list(const unsigned long long* __restrict__ bitmap, uint32_t nwords,
                                                              const u256* __restrict__ sums, uint32_t m, uint32_t sums_mont,
                                                              WitnessDev* rep) {
  if (rep->noncanonical_count || !rep->bad_count) return;   // uniform
  __shared__ uint32_t scan[WITNESS_LANES];
  const uint32_t t = threadIdx.x;
  uint32_t found = 0;
  for (uint32_t base = 0; base < nwords && found < WITNESS_LIST; base += WITNESS_LANES) {
    const uint32_t idx = base + t;
    const uint64_t w = idx < nwords ? bitmap[idx] : 0;
    const uint32_t c = (uint32_t)__popcll(w);
    scan[t] = c;
    __syncthreads();
    for (uint32_t off = 1; off < WITNESS_LANES; off <<= 1) {   // inclusive prefix sum
      const uint32_t v = t >= off ? scan[t - off] : 0;
      __syncthreads();
      scan[t] += v;
      __syncthreads();
    }
    const uint32_t before = found + scan[t] - c;
    found += scan[WITNESS_LANES - 1];
    __syncthreads();   // scan is rewritten by the next trip
    if (!c || before >= WITNESS_LIST) continue;
    witness_take(w, idx, before, rep->list);
    if (before == 0) {   // this lane holds the smallest failing constraint: its three sums, in standard form
      const uint32_t i = 64u * idx + (uint32_t)__ffsll((long long)w) - 1u;
      const u256 a = sums[i], b = sums[(size_t)m + i], cc = sums[2 * (size_t)m + i];
      rep->az = sums_mont ? Fr::from_mont(a) : a;
      rep->bz = sums_mont ? Fr::from_mont(b) : b;
      rep->cz = sums_mont ? Fr::from_mont(cc) : cc;
    }
  }
}

}  // namespace

struct g16_r1cs {
  int device = 0;
  uint32_t nvars = 0, ncons = 0;
  size_t nnz = 0, ndict = 0;
  Building<g16_spmat, g16_spmat_destroy> m;
};

extern "C" void g16_r1cs_destroy(g16_r1cs* r) {
  if (!r) return;
  (void)hipSetDevice(r->device);
  delete r;
}

extern "C" int32_t g16_r1cs_info(const g16_r1cs* r, size_t out[4]) {
  if (!r || !out) return G16_EINVAL;
  out[0] = r->nvars, out[1] = r->ncons, out[2] = r->nnz, out[3] = r->ndict;
  return G16_OK;
}

namespace {

int32_t r1cs_fail(g16_ctx* ctx, const std::string& msg) {
  ctx->err = "g16_r1cs_create: " + msg;
  return G16_EINVAL;
}

int32_t r1cs_validate(g16_ctx* ctx, const g16_r1cs_desc* d, g16_r1cs** out) {
  if (!d || !out) return r1cs_fail(ctx, "null argument");
  for (int k = 0; k < 3; ++k)
    if (d->nnz[k] && (!d->row[k] || !d->col[k] || !d->val[k])) return r1cs_fail(ctx, "null matrix pointer");
  if (d->flags != G16_SCALARS_MONT && d->flags != G16_SCALARS_STD)
    return r1cs_fail(ctx, "r1cs flags must be G16_SCALARS_MONT or _STD");
  if (d->flavour != G16_FLAVOUR_SNARKJS && d->flavour != G16_FLAVOUR_JENSGROTH) return r1cs_fail(ctx, "unknown flavour");
  if (d->nvars == 0 || d->nvars >= (1u << 27) || d->npubs >= d->nvars)
    return r1cs_fail(ctx, "bad wire counts (0 < nvars < 2^27, npubs < nvars)");
  if (d->nconstraints >= (1u << 28)) return r1cs_fail(ctx, "too many constraints (< 2^28)");
  for (int k = 0; k < 3; ++k)
    for (size_t i = 0; i < d->nnz[k]; ++i) {
      if (d->row[k][i] >= d->nconstraints || d->col[k][i] >= d->nvars)
        return r1cs_fail(ctx, "r1cs matrix " + std::to_string(k) + " entry " + std::to_string(i) + " out of range");
      u256 v;
      memcpy(&v, (const char*)d->val[k] + 32 * i, 32);
      if (!Fr::is_canonical(v))
        return r1cs_fail(ctx, "r1cs matrix " + std::to_string(k) + " entry " + std::to_string(i) +
                                  ": value is not canonical (>= r)");
    }
  return G16_OK;
}

// A, B and C as one matrix of virtual rows 3 i + k, values in Montgomery form
int32_t r1cs_create(g16_ctx* ctx, const g16_r1cs_desc* d, g16_r1cs** out) {
  const bool mont = d->flags == G16_SCALARS_MONT;
  const size_t nnz = d->nnz[0] + d->nnz[1] + d->nnz[2];
  std::vector<uint32_t> vrow(nnz ? nnz : 1), col(nnz ? nnz : 1);
  std::vector<u256> val(nnz ? nnz : 1);
  size_t e = 0;
  for (uint32_t k = 0; k < 3; ++k)
    for (size_t i = 0; i < d->nnz[k]; ++i, ++e) {
      vrow[e] = 3 * d->row[k][i] + k, col[e] = d->col[k][i];
      memcpy(&val[e], (const char*)d->val[k] + 32 * i, 32);
      if (!mont) val[e] = Fr::to_mont(val[e]);
    }
  Building<g16_r1cs, g16_r1cs_destroy> r(new (std::nothrow) g16_r1cs());
  if (!r) return G16_ENOMEM;
  r->device = ctx->device, r->nvars = d->nvars, r->ncons = d->nconstraints, r->nnz = nnz;
  g16_spmat* built = nullptr;
  const int32_t rc = g16_spmat_create(ctx, 3, d->nconstraints, nnz, vrow.data(), 4, col.data(), 4, val.data(), 32, &built);
  r->m.reset(built);
  if (rc) return rc;
  size_t info[10];
  g16_spmat_info(built, info);
  r->ndict = info[0];
  *out = r.release();
  return G16_OK;
}

inline uint32_t grid_of(size_t n) { return (uint32_t)((n + WITNESS_BLOCK - 1) / WITNESS_BLOCK); }

}  // namespace

extern "C" int32_t g16_r1cs_create(g16_ctx* ctx, const g16_r1cs_desc* desc, g16_r1cs** out) {
  if (!ctx) return G16_EINVAL;
  if (out) *out = nullptr;
  if (int32_t rc = r1cs_validate(ctx, desc, out)) return rc;
  CTX_ENTER(ctx);
  try {   // the matrices are arranged in host vectors: no exception may cross the C ABI
    return r1cs_create(ctx, desc, out);
  } catch (const std::bad_alloc&) {
    ctx->err = "out of host memory while arranging the matrices";
    return G16_ENOMEM;
  }
}

extern "C" int32_t g16_witness_check(g16_ctx* ctx, const g16_r1cs* r, const void* witness, uint32_t flags,
                                     g16_witness_report* out) {
  if (!ctx) return G16_EINVAL;
  static const char who[] = "g16_witness_check: ";
  if (!r || !witness || !out) {
    ctx->err = std::string(who) + "null argument";
    return G16_EINVAL;
  }
  if (flags & ~(G16_SCALARS_MONT | G16_SCALARS_DEVICE)) {
    ctx->err = std::string(who) + "flags must be G16_SCALARS_MONT or _STD, optionally | G16_SCALARS_DEVICE";
    return G16_EINVAL;
  }
  if (r->device != ctx->device) {
    ctx->err = std::string(who) + "the constraint system belongs to another device";
    return G16_EINVAL;
  }
  CTX_ENTER(ctx);
  const bool mont = flags & G16_SCALARS_MONT, on_device = flags & G16_SCALARS_DEVICE;
  const uint32_t nv = r->nvars, m = r->ncons;
  const size_t nwords = witness_words(m);
  // the workspace of the call, in the context's per-proof buffer: [witness] | A z | B z | C z | bitmap | report
  const size_t w_bytes = on_device ? 0 : (size_t)nv * 32, sums_bytes = 3 * (size_t)m * 32;
  const size_t map_bytes = (nwords * 8 + 31) / 32 * 32;
  int32_t rc;
  if ((rc = ensure(ctx, ctx->prove, w_bytes + sums_bytes + map_bytes + sizeof(WitnessDev)))) return rc;
  char* const base = (char*)ctx->prove.p();
  u256* const d_sums = (u256*)(base + w_bytes);
  unsigned long long* const d_map = (unsigned long long*)(base + w_bytes + sums_bytes);
  WitnessDev* const d_rep = (WitnessDev*)(base + w_bytes + sums_bytes + map_bytes);
  const u256* d_w = (const u256*)witness;
  SyncOnExit drain{ctx->stream};   // every error exit below leaves with the stream drained: the caller's buffer is not being read
  if (!on_device) {
    HIPCHK(ctx, hipMemcpyAsync(base, witness, w_bytes, hipMemcpyHostToDevice, ctx->stream));
    d_w = (const u256*)base;
  }
  HIPCHK(ctx, hipMemsetAsync(d_rep, 0xff, WITNESS_DEV_ONES, ctx->stream));
  HIPCHK(ctx, hipMemsetAsync((char*)d_rep + WITNESS_DEV_ONES, 0, sizeof(WitnessDev) - WITNESS_DEV_ONES, ctx->stream));
  u256 one = Fr::one();   // R mod r; the standard form of 1 is the integer
  if (!mont) {
    one = Fr::zero();
    one.v[0] = 1;
  }
  KLAUNCH(ctx, "witness_canonical", witness_canonical, grid_of(nv), WITNESS_BLOCK, 0, d_w, nv, one, d_rep);
  HIPCHK(ctx, hipGetLastError());
  if (m) {
    const uint32_t sums_mont = (mont || r->ndict) ? 1u : 0u;
    if ((rc = g16_spmat_apply(ctx, r->m.get(), d_w, mont ? 1u : 0u, d_sums, false))) return rc;
    KLAUNCH(ctx, "witness_rows", witness_rows, grid_of(m), WITNESS_BLOCK, 0, (const u256*)d_sums, m, sums_mont, d_map, d_rep);
    KLAUNCH(ctx, "witness_list", witness_list, 1, WITNESS_LANES, 0, (const unsigned long long*)d_map, (uint32_t)nwords,
            (const u256*)d_sums, m, sums_mont, d_rep);
  }
  hipError_t launched = hipGetLastError();
  WitnessDev got;
  if (launched == hipSuccess)
    launched = hipMemcpyAsync(&got, d_rep, sizeof got, hipMemcpyDeviceToHost, ctx->stream);
  const hipError_t drained = hipStreamSynchronize(ctx->stream);   // the one wait of a call that succeeds
  HIPCHK(ctx, launched);
  HIPCHK(ctx, drained);

  memset(out, 0, sizeof *out);
  constexpr size_t NONE = (size_t)-1;
  out->noncanonical_count = got.noncanonical_count;
  out->first_noncanonical = got.noncanonical_count ? (size_t)got.first_noncanonical : NONE;
  for (uint32_t k = 0; k < WITNESS_LIST; ++k) out->first_bad[k] = NONE;
  if (got.noncanonical_count) {
    out->failed |= G16_WITNESS_CANONICAL;
    out->constraints = -1;
  } else {
    out->bad_count = got.bad_count;
    out->constraints = got.bad_count ? 0 : 1;
    if (got.bad_count) {
      out->failed |= G16_WITNESS_CONSTRAINTS;
      for (uint32_t k = 0; k < WITNESS_LIST; ++k)
        if (got.list[k] != WITNESS_NONE) out->first_bad[k] = got.list[k];
      memcpy(out->az, &got.az, 32), memcpy(out->bz, &got.bz, 32), memcpy(out->cz, &got.cz, 32);
    }
  }
  if (got.one_bad) out->failed |= G16_WITNESS_ONE;
  return G16_OK;
}
