// Fake circuit-specific trusted setup on the device (reference groth16/fake_setup.nim:201-326): the kernels over
// setup.cuh and the host layer of g16_fake_setup, g16_lagrange_fr, g16_powers_fr and g16_setup_log2_domain
// (include/g16hip.h).  The group side -- every `y ** gen1` / `y ** gen2` -- is fixed_base_device (msm_stage.cuh), the
// sparse column sums are the row-balanced kernel of buildABC over the transposed matrices (spmv.hip); what is new here
// is that the scalars between them never leave HBM.
#include <new>

#include "g16_internal.hpp"
#include "ec.cuh"
#include "setup.cuh"

using namespace g16;

namespace {

// out[i] = c * x_i (powers) or c * x_i / (tau - x_i) (lagrange), x_i = w0 * s^i, i < count; thread t owns the run
// [t * SETUP_RUN, (t + 1) * SETUP_RUN) cut at count.  *first_zero (0xffffffff on entry): the smallest i with tau == x_i.
template <bool LAGRANGE>
__global__ void __launch_bounds__(SETUP_BLOCK) setup_geometric(u256 w0, u256 s, u256 c, u256 tau, uint32_t count,
                                                               u256* __restrict__ out, uint32_t* first_zero) {
  const uint32_t t = blockIdx.x * SETUP_BLOCK + threadIdx.x;
  if (t >= (count + SETUP_RUN - 1) / SETUP_RUN) return;
  const uint32_t i0 = t * SETUP_RUN;   // count <= 2^29: no overflow
  const uint32_t len = count - i0 < (uint32_t)SETUP_RUN ? count - i0 : (uint32_t)SETUP_RUN;
  const u256 x0 = Fr::mul(w0, setup_pow_u32(s, i0));
  const uint32_t z = setup_geom_run<SETUP_RUN, LAGRANGE>(x0, s, c, tau, len, out + i0);
  if (LAGRANGE && z < (uint32_t)SETUP_RUN) atomicMin(first_zero, i0 + z);
}

// out[j] = (beta A_j + alpha B_j + C_j) / (j <= npubs ? gamma : delta); sums = A | B | C column sums, nvars each
__global__ void __launch_bounds__(SETUP_BLOCK) setup_combine_wires(const u256* __restrict__ sums, u256 alpha, u256 beta,
                                                                   u256 gamma_inv, u256 delta_inv, uint32_t nvars,
                                                                   uint32_t npubs, u256* __restrict__ out) {
  const uint32_t j = blockIdx.x * SETUP_BLOCK + threadIdx.x;
  if (j >= nvars) return;
  out[j] = setup_combine(sums[j], sums[(size_t)nvars + j], sums[2 * (size_t)nvars + j], alpha, beta, gamma_inv,
                         delta_inv, j, npubs);
}

constexpr uint32_t SETUP_MAX_LOG2 = 28;                      // the two-adicity of Fr (math/domain.nim:26)
constexpr size_t SETUP_MAX_COUNT = size_t(1) << 29;          // a run's first index is an exponent below 2^29

int32_t launch_geometric(g16_ctx* ctx, bool lagrange, const u256& w0, const u256& s, const u256& c, const u256& tau,
                         size_t count, u256* d_out, uint32_t* d_first_zero) {
  if (!count) return G16_OK;
  const uint32_t threads = (uint32_t)((count + SETUP_RUN - 1) / SETUP_RUN);
  const uint32_t grid = (threads + SETUP_BLOCK - 1) / SETUP_BLOCK;
  if (lagrange)
    KLAUNCH(ctx, "setup_lagrange", setup_geometric<true>, grid, SETUP_BLOCK, 0, w0, s, c, tau, (uint32_t)count, d_out,
            d_first_zero);
  else
    KLAUNCH(ctx, "setup_powers", setup_geometric<false>, grid, SETUP_BLOCK, 0, w0, s, c, tau, (uint32_t)count, d_out,
            d_first_zero);
  HIPCHK(ctx, hipGetLastError());
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

// tau^(2^k)
u256 pow2k(u256 x, uint32_t k) {
  for (uint32_t i = 0; i < k; ++i) x = Fr::sqr(x);
  return x;
}
// (tau^(2^k) - 1) / 2^k: the factor every L_j(tau) of the 2^k domain shares (math/poly.nim:246-249)
u256 vanishing_over_n(const u256& tau, uint32_t k) {
  u256 z = Fr::sub(pow2k(tau, k), Fr::one());
  for (uint32_t i = 0; i < k; ++i) z = Fr::div2(z);
  return z;
}

int32_t tau_in_domain(g16_ctx* ctx, uint32_t log2n, uint64_t first, uint64_t step, uint32_t element) {
  char msg[160];
  snprintf(msg, sizeof msg, "tau lies in the domain: it equals omega^%llu of the 2^%u domain (element %u of the request)",
           (unsigned long long)(first + step * element), log2n, element);
  ctx->err = msg;
  return G16_EINVAL;
}

}  // namespace

// the geometric-sequence kernel for the circuit setup (circuit_setup.hip): its twiddles and coset factors
int32_t g16_setup_geometric(g16_ctx* ctx, bool lagrange, const u256& w0, const u256& s, const u256& c, const u256& tau,
                            size_t count, u256* d_out, uint32_t* d_first_zero) {
  return launch_geometric(ctx, lagrange, w0, s, c, tau, count, d_out, d_first_zero);
}

// ceilingLog2(n + p + 1) (fake_setup.nim:203-206): pure
extern "C" int32_t g16_setup_log2_domain(const g16_setup_desc* desc, uint32_t* log2_domain) {
  if (!desc || !log2_domain) return G16_EINVAL;
  *log2_domain = setup_log2_domain(desc->nconstraints, desc->npubs);
  return G16_OK;
}

// out[i] = scale * L_{first + step i}(tau) on the 2^log2n domain (math/poly.nim:242-250); host pointers, Montgomery
extern "C" int32_t g16_lagrange_fr(g16_ctx* ctx, uint32_t log2n, uint32_t first, uint32_t step, size_t count,
                                   const void* tau, const void* scale, void* out) {
  if (!ctx) return G16_EINVAL;
  if (!tau || (count && !out)) {
    ctx->err = "null pointer argument";
    return G16_EINVAL;
  }
  if (log2n > SETUP_MAX_LOG2) {
    ctx->err = "log2n out of range (must be <= 28)";
    return G16_EINVAL;
  }
  if (count && (count > (size_t(1) << log2n) || (uint64_t)first + (uint64_t)step * (count - 1) >= (uint64_t(1) << log2n))) {
    ctx->err = "first + step * (count - 1) lies outside the domain";
    return G16_EINVAL;
  }
  u256 t, sc = Fr::one();
  if (!load_scalar(tau, true, t) || (scale && !load_scalar(scale, true, sc))) {
    ctx->err = "tau or scale is not canonical (>= r)";
    return G16_EINVAL;
  }
  if (!count) return G16_OK;
  CTX_ENTER(ctx);
  const u256 omega = setup_omega(log2n);
  const u256 w0 = setup_pow_u32(omega, first), s = setup_pow_u32(omega, step);
  const u256 c = Fr::mul(sc, vanishing_over_n(t, log2n));
  DevMem<u256> d_out;
  DevMem<uint32_t> d_flag;
  SyncOnExit sync{ctx->stream};
  HIPCHK(ctx, dev_alloc(d_out, count * 32));
  HIPCHK(ctx, dev_alloc(d_flag, 4));
  HIPCHK(ctx, hipMemsetAsync(d_flag.get(), 0xff, 4, ctx->stream));
  if (int32_t rc = launch_geometric(ctx, true, w0, s, c, t, count, d_out.get(), d_flag.get())) return rc;
  uint32_t flag = 0;
  HIPCHK(ctx, hipMemcpyAsync(out, d_out.get(), count * 32, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(&flag, d_flag.get(), 4, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  if (flag != 0xffffffffu) return tau_in_domain(ctx, log2n, first, step, flag);
  return G16_OK;
}

// out[i] = scale * base^i: the JensGroth H scalars (fake_setup.nim:290-294); host pointers, Montgomery
extern "C" int32_t g16_powers_fr(g16_ctx* ctx, const void* base, const void* scale, size_t count, void* out) {
  if (!ctx) return G16_EINVAL;
  if (!base || (count && !out)) {
    ctx->err = "null pointer argument";
    return G16_EINVAL;
  }
  if (count > SETUP_MAX_COUNT) {
    ctx->err = "count too large (must be <= 2^29)";
    return G16_EINVAL;
  }
  u256 b, sc = Fr::one();
  if (!load_scalar(base, true, b) || (scale && !load_scalar(scale, true, sc))) {
    ctx->err = "base or scale is not canonical (>= r)";
    return G16_EINVAL;
  }
  if (!count) return G16_OK;
  CTX_ENTER(ctx);
  DevMem<u256> d_out;
  SyncOnExit sync{ctx->stream};
  HIPCHK(ctx, dev_alloc(d_out, count * 32));
  if (int32_t rc = launch_geometric(ctx, false, Fr::one(), b, sc, Fr::zero(), count, d_out.get(), nullptr)) return rc;
  HIPCHK(ctx, hipMemcpyAsync(out, d_out.get(), count * 32, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return G16_OK;
}

namespace {

struct SetupScalars {
  u256 alpha, beta, gamma, delta, tau;   // Montgomery
};

// everything g16_fake_setup rejects before it queues anything
int32_t setup_validate(g16_ctx* ctx, const g16_setup_desc* d, const g16_setup_points* o, uint32_t& log2_dom,
                       SetupScalars& tw) {
  auto bad = [&](const char* msg) {
    ctx->err = msg;
    return G16_EINVAL;
  };
  if (!d || !o) return bad("null pointer argument");
  if (!d->alpha || !d->beta || !d->gamma || !d->delta || !d->tau) return bad("null toxic-waste pointer");
  for (int k = 0; k < 3; ++k)
    if (d->nnz[k] && (!d->row[k] || !d->col[k] || !d->val[k])) return bad("null matrix pointer");
  if (!o->alpha1 || !o->beta1 || !o->delta1 || !o->beta2 || !o->gamma2 || !o->delta2 || !o->pointsIC || !o->pointsA1 ||
      !o->pointsB1 || !o->pointsB2 || !o->pointsH1 || (d->nvars > d->npubs + 1 && !o->pointsC1))
    return bad("null output pointer");
  if (d->flavour != G16_FLAVOUR_JENSGROTH && d->flavour != G16_FLAVOUR_SNARKJS) return bad("unknown flavour");
  if (d->flags != G16_SCALARS_MONT && d->flags != G16_SCALARS_STD) return bad("flags must be G16_SCALARS_MONT or _STD");
  if (d->nvars <= d->npubs) return bad("nvars must exceed npubs (wire 0 is the constant one)");
  log2_dom = setup_log2_domain(d->nconstraints, d->npubs);
  if (log2_dom + (d->flavour == G16_FLAVOUR_SNARKJS ? 1u : 0u) > SETUP_MAX_LOG2)
    return bad("domain too large (the domain, doubled for the snarkjs flavour, must not exceed 2^28)");
  const bool mont = d->flags == G16_SCALARS_MONT;
  if (!load_scalar(d->alpha, mont, tw.alpha) || !load_scalar(d->beta, mont, tw.beta) ||
      !load_scalar(d->gamma, mont, tw.gamma) || !load_scalar(d->delta, mont, tw.delta) ||
      !load_scalar(d->tau, mont, tw.tau))
    return bad("toxic-waste scalar is not canonical (>= r)");
  if (Fr::is_zero(tw.gamma) || Fr::is_zero(tw.delta)) return bad("gamma and delta must not be zero");
  char msg[128];
  for (int k = 0; k < 3; ++k)
    for (size_t i = 0; i < d->nnz[k]; ++i) {
      if (d->row[k][i] >= d->nconstraints || d->col[k][i] >= d->nvars) {
        snprintf(msg, sizeof msg, "matrix %d entry %zu out of range", k, i);
        return bad(msg);
      }
      u256 v;
      memcpy(&v, (const char*)d->val[k] + 32 * i, 32);
      if (!Fr::is_canonical(v)) {
        snprintf(msg, sizeof msg, "matrix %d entry %zu: value is not canonical (>= r)", k, i);
        return bad(msg);
      }
    }
  return G16_OK;
}

template <class C>
int32_t setup_fixed_base(g16_ctx* ctx, const void* d_scalars, size_t n, void* d_out) {
  constexpr int g = sizeof(typename C::Aff) == sizeof(g1_aff) ? 0 : 1;
  if (int32_t rc = ensure(ctx, ctx->fb_table[g], 32 * 255 * sizeof(typename C::Aff))) return rc;
  if (int32_t rc = fixed_base_device<C>(ctx, ctx->fb_table[g].p(), ctx->fb_ready[g], d_scalars, 1, n, d_out)) return rc;
  ctx->fb_ready[g] = true;
  return G16_OK;
}

int32_t fake_setup(g16_ctx* ctx, const g16_setup_desc* d, g16_setup_points* o, uint32_t log2_dom, const SetupScalars& tw) {
  const bool mont = d->flags == G16_SCALARS_MONT;
  const uint32_t nvars = d->nvars, npubs = d->npubs, ncons = d->nconstraints;
  const size_t dom = size_t(1) << log2_dom;
  // owners first, the drain of the stream that uses them last (released in reverse order)
  Building<g16_spmat, g16_spmat_destroy> mat[3];
  DevMem<u256> d_lag, d_sums, d_comb, d_h, d_spec;
  DevMem<uint32_t> d_flags;
  DevMem<g1_aff> d_a1, d_b1, d_icc, d_h1, d_spec1;
  DevMem<g2_aff> d_b2, d_spec2;
  SyncOnExit sync{ctx->stream};
  int32_t rc;

  // 1. the triplets, transposed: row = wire, col = constraint; A with snarkjs's dummy rows (n + i, wire i, 1) for the
  //    public IO (fake_setup.nim:182-185).  Values in standard form stay as they are: the Lagrange values then carry
  //    one more factor R, and the Montgomery products of the column sums come out in Montgomery form.
  for (int k = 0; k < 3; ++k) {
    g16_spmat* built = nullptr;
    if (k == 0) {
      const size_t nnz = d->nnz[0], tot = nnz + npubs + 1;
      std::vector<uint32_t> wire(tot), con(tot);
      std::vector<u256> val(tot);
      if (nnz) {
        memcpy(wire.data(), d->col[0], nnz * 4);
        memcpy(con.data(), d->row[0], nnz * 4);
        memcpy(val.data(), d->val[0], nnz * 32);
      }
      u256 one = Fr::zero();
      one.v[0] = 1;
      if (mont) one = Fr::one();
      for (uint32_t i = 0; i <= npubs; ++i) wire[nnz + i] = i, con[nnz + i] = ncons + i, val[nnz + i] = one;
      rc = g16_spmat_create(ctx, 1, nvars, tot, wire.data(), 4, con.data(), 4, val.data(), 32, &built);
    } else {
      rc = g16_spmat_create(ctx, 1, nvars, d->nnz[k], d->col[k], 4, d->row[k], 4, d->val[k], 32, &built);
    }
    if (rc) return rc;
    mat[k].reset(built);
  }
  HIPCHK(ctx, dev_alloc(d_lag, dom * 32));
  HIPCHK(ctx, dev_alloc(d_sums, 3 * (size_t)nvars * 32));
  HIPCHK(ctx, dev_alloc(d_comb, (size_t)nvars * 32));
  HIPCHK(ctx, dev_alloc(d_h, dom * 32));
  HIPCHK(ctx, dev_alloc(d_spec, 6 * 32));
  HIPCHK(ctx, dev_alloc(d_flags, 8));
  HIPCHK(ctx, dev_alloc(d_a1, (size_t)nvars * sizeof(g1_aff)));
  HIPCHK(ctx, dev_alloc(d_b1, (size_t)nvars * sizeof(g1_aff)));
  HIPCHK(ctx, dev_alloc(d_b2, (size_t)nvars * sizeof(g2_aff)));
  HIPCHK(ctx, dev_alloc(d_icc, (size_t)nvars * sizeof(g1_aff)));
  HIPCHK(ctx, dev_alloc(d_h1, dom * sizeof(g1_aff)));
  HIPCHK(ctx, dev_alloc(d_spec1, 3 * sizeof(g1_aff)));
  HIPCHK(ctx, dev_alloc(d_spec2, 3 * sizeof(g2_aff)));
  HIPCHK(ctx, hipMemsetAsync(d_flags.get(), 0xff, 8, ctx->stream));

  // 2. L_j(tau), j < dom (fake_setup.nim:254-256 through math/poly.nim:242-250)
  const u256 c_dom = vanishing_over_n(tw.tau, log2_dom);
  if ((rc = launch_geometric(ctx, true, Fr::one(), setup_omega(log2_dom), mont ? c_dom : Fr::to_mont(c_dom), tw.tau, dom,
                             d_lag.get(), d_flags.get())))
    return rc;
  // 3. the column sums A | B | C
  for (int k = 0; k < 3; ++k)
    if ((rc = g16_spmat_apply(ctx, mat[k].get(), d_lag.get(), 1, d_sums.get() + (size_t)k * nvars))) return rc;
  // 4. the combinations for pointsIC and pointsC1
  const u256 gamma_inv = Fr::inv(tw.gamma), delta_inv = Fr::inv(tw.delta);
  KLAUNCH(ctx, "setup_combine", setup_combine_wires, (nvars + SETUP_BLOCK - 1) / SETUP_BLOCK, SETUP_BLOCK, 0,
          (const u256*)d_sums.get(), tw.alpha, tw.beta, gamma_inv, delta_inv, nvars, npubs, d_comb.get());
  HIPCHK(ctx, hipGetLastError());
  // 5. the H scalars of the flavour
  if (d->flavour == G16_FLAVOUR_JENSGROTH) {   // delta^-1 Z(tau) tau^i (fake_setup.nim:290-294)
    const u256 c = Fr::mul(delta_inv, Fr::sub(pow2k(tw.tau, log2_dom), Fr::one()));
    rc = launch_geometric(ctx, false, Fr::one(), tw.tau, c, Fr::zero(), dom, d_h.get(), nullptr);
  } else {   // delta^-1 L_{2i+1}(tau) on the doubled domain (fake_setup.nim:299-304)
    const u256 w2 = setup_omega(log2_dom + 1);
    const u256 c = Fr::mul(delta_inv, vanishing_over_n(tw.tau, log2_dom + 1));
    rc = launch_geometric(ctx, true, w2, Fr::sqr(w2), c, tw.tau, dom, d_h.get(), d_flags.get() + 1);
  }
  if (rc) return rc;
  // 6. `y ** gen1` / `y ** gen2` (fake_setup.nim:258-261, 273-277, 290-302)
  const u256 spec[6] = {tw.alpha, tw.beta, tw.delta, tw.beta, tw.gamma, tw.delta};
  HIPCHK(ctx, hipMemcpyAsync(d_spec.get(), spec, sizeof spec, hipMemcpyHostToDevice, ctx->stream));
  const u256 *sA = d_sums.get(), *sB = d_sums.get() + nvars;
  if ((rc = setup_fixed_base<G1>(ctx, sA, nvars, d_a1.get()))) return rc;
  if ((rc = setup_fixed_base<G1>(ctx, sB, nvars, d_b1.get()))) return rc;
  if ((rc = setup_fixed_base<G2>(ctx, sB, nvars, d_b2.get()))) return rc;
  if ((rc = setup_fixed_base<G1>(ctx, d_comb.get(), nvars, d_icc.get()))) return rc;
  if ((rc = setup_fixed_base<G1>(ctx, d_h.get(), dom, d_h1.get()))) return rc;
  if ((rc = setup_fixed_base<G1>(ctx, d_spec.get(), 3, d_spec1.get()))) return rc;
  if ((rc = setup_fixed_base<G2>(ctx, d_spec.get() + 3, 3, d_spec2.get()))) return rc;
  // 7. the points to the caller
  auto down = [&](void* dst, const void* src, size_t bytes) {
    return bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream) : hipSuccess;
  };
  HIPCHK(ctx, down(o->pointsA1, d_a1.get(), (size_t)nvars * sizeof(g1_aff)));
  HIPCHK(ctx, down(o->pointsB1, d_b1.get(), (size_t)nvars * sizeof(g1_aff)));
  HIPCHK(ctx, down(o->pointsB2, d_b2.get(), (size_t)nvars * sizeof(g2_aff)));
  HIPCHK(ctx, down(o->pointsIC, d_icc.get(), ((size_t)npubs + 1) * sizeof(g1_aff)));
  HIPCHK(ctx, down(o->pointsC1, d_icc.get() + npubs + 1, ((size_t)nvars - npubs - 1) * sizeof(g1_aff)));
  HIPCHK(ctx, down(o->pointsH1, d_h1.get(), dom * sizeof(g1_aff)));
  HIPCHK(ctx, down(o->alpha1, d_spec1.get(), sizeof(g1_aff)));
  HIPCHK(ctx, down(o->beta1, d_spec1.get() + 1, sizeof(g1_aff)));
  HIPCHK(ctx, down(o->delta1, d_spec1.get() + 2, sizeof(g1_aff)));
  HIPCHK(ctx, down(o->beta2, d_spec2.get(), sizeof(g2_aff)));
  HIPCHK(ctx, down(o->gamma2, d_spec2.get() + 1, sizeof(g2_aff)));
  HIPCHK(ctx, down(o->delta2, d_spec2.get() + 2, sizeof(g2_aff)));
  uint32_t flags[2] = {0, 0};
  HIPCHK(ctx, hipMemcpyAsync(flags, d_flags.get(), 8, hipMemcpyDeviceToHost, ctx->stream));
  // 8.
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  if (flags[0] != 0xffffffffu) return tau_in_domain(ctx, log2_dom, 0, 1, flags[0]);
  if (flags[1] != 0xffffffffu) return tau_in_domain(ctx, log2_dom + 1, 1, 2, flags[1]);
  return G16_OK;
}

}  // namespace

// fakeCircuitSetup (fake_setup.nim:201-326) minus ZKey.coeffs, which is a rearrangement of the input (r1csToCoeffs, :46-65)
extern "C" int32_t g16_fake_setup(g16_ctx* ctx, const g16_setup_desc* desc, g16_setup_points* out) {
  if (!ctx) return G16_EINVAL;
  uint32_t log2_dom = 0;
  SetupScalars tw;
  if (int32_t rc = setup_validate(ctx, desc, out, log2_dom, tw)) return rc;
  CTX_ENTER(ctx);
  try {   // the dummy rows of A are appended in host vectors: no exception may cross the C ABI
    return fake_setup(ctx, desc, out, log2_dom, tw);
  } catch (const std::bad_alloc&) {
    ctx->err = "out of host memory while arranging the matrices";
    return G16_ENOMEM;
  }
}
