// Scaling an array of points by one scalar or by a scalar per point (include/g16hip.h, "scaling an array of points"): host
// layer of g16_points_scale_g1/g2 and g16_points_scale_each_g1/g2, and the job every caller of scale_uniform_device builds first.  The schedule of the G1 ladder is
// made here, once per call, from the scalar (scale_plan.hpp); kernels: scale.cuh.
#include "g16_internal.hpp"
#include "ec.cuh"
#include "scale_plan.hpp"

using namespace g16;

// The job of k (standard form, canonical): the plan of k uploaded into d_steps (room for ScalePlan::MAX_STEPS words; the
// host copy `plan` must live until the stream has taken it), and k itself for the G2 ladder.
int32_t g16_scale_job(g16_ctx* ctx, const u256& k_std, ScalePlan& plan, uint32_t* d_steps, ScaleJob& job) {
  U256 k;
  for (int i = 0; i < 4; ++i) k.v[i] = (uint64_t)k_std.v[2 * i] | (uint64_t)k_std.v[2 * i + 1] << 32;
  bool ok = false;
  plan = make_scale_plan(k, &ok);
  if (!ok || !scale_plan_is(plan, k)) {   // cannot happen for k < r: the halves stay below 2^128
    ctx->err = "scale plan: the decomposition of the scalar failed its own check";
    return G16_ESELFTEST;
  }
  if (plan.nsteps)
    HIPCHK(ctx, hipMemcpyAsync(d_steps, plan.step, sizeof(ScaleStep) * (size_t)plan.nsteps, hipMemcpyHostToDevice,
                               ctx->stream));
  job.d_steps = d_steps;
  job.nsteps = (uint32_t)plan.nsteps, job.tail_dbls = (uint32_t)plan.tail_dbls;
  for (int q = 0; q < 8; ++q) job.k_std[q] = k_std.v[q];
  return G16_OK;
}

namespace {

template <class C>
int32_t points_scale(g16_ctx* ctx, const void* points, size_t n, const void* k, uint32_t flags, void* out) {
  if (!ctx) return G16_EINVAL;
  auto bad = [&](const char* msg) {
    ctx->err = std::string("g16_points_scale: ") + msg;
    return G16_EINVAL;
  };
  if (!k || (n && (!points || !out))) return bad("null pointer argument");
  if (flags != G16_SCALARS_MONT && flags != G16_SCALARS_STD) return bad("flags must be G16_SCALARS_MONT or G16_SCALARS_STD");
  if (n >= (size_t(1) << 31)) return bad("n out of range (must be < 2^31)");
  u256 kv;
  memcpy(&kv, k, 32);
  if (!Fr::is_canonical(kv)) return bad("the scalar is not canonical (>= r)");
  if (flags == G16_SCALARS_MONT) kv = Fr::from_mont(kv);
  if (!n) return G16_OK;
  CTX_ENTER(ctx);
  ScalePlan plan;   // lives until the wait below
  ScaleJob job;
  DevMem<typename C::Aff> d_pts;
  DevMem<uint32_t> d_steps;
  SyncOnExit drain{ctx->stream};
  HIPCHK(ctx, dev_alloc(d_pts, n * sizeof(typename C::Aff)));
  HIPCHK(ctx, dev_alloc(d_steps, ScalePlan::MAX_STEPS * sizeof(uint32_t)));
  HIPCHK(ctx, hipMemcpyAsync(d_pts.get(), points, n * sizeof(typename C::Aff), hipMemcpyHostToDevice, ctx->stream));
  int32_t rc;
  if ((rc = g16_scale_job(ctx, kv, plan, d_steps.get(), job))) return rc;
  if ((rc = scale_uniform_device<C>(ctx, d_pts.get(), n, job, d_pts.get()))) return rc;
  HIPCHK(ctx, hipMemcpyAsync(out, d_pts.get(), n * sizeof(typename C::Aff), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return G16_OK;
}

// a scalar per point: the scalars are checked here, the split of each is the lane's own work (scale_each.cuh)
template <class C>
int32_t points_scale_each(g16_ctx* ctx, const void* points, size_t n, const void* scalars, uint32_t flags, void* out) {
  if (!ctx) return G16_EINVAL;
  auto bad = [&](const std::string& msg) {
    ctx->err = "g16_points_scale_each: " + msg;
    return G16_EINVAL;
  };
  if (n && (!points || !scalars || !out)) return bad("null pointer argument");
  if (flags != G16_SCALARS_MONT && flags != G16_SCALARS_STD) return bad("flags must be G16_SCALARS_MONT or G16_SCALARS_STD");
  if (n >= (size_t(1) << 31)) return bad("n out of range (must be < 2^31)");
  for (size_t i = 0; i < n; ++i) {
    u256 kv;
    memcpy(&kv, (const char*)scalars + 32 * i, 32);
    if (!Fr::is_canonical(kv)) return bad("scalar " + std::to_string(i) + " is not canonical (>= r)");
  }
  if (!n) return G16_OK;
  CTX_ENTER(ctx);
  DevMem<typename C::Aff> d_pts;
  DevMem<u256> d_k;
  SyncOnExit drain{ctx->stream};
  HIPCHK(ctx, dev_alloc(d_pts, n * sizeof(typename C::Aff)));
  HIPCHK(ctx, dev_alloc(d_k, n * sizeof(u256)));
  HIPCHK(ctx, hipMemcpyAsync(d_pts.get(), points, n * sizeof(typename C::Aff), hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(d_k.get(), scalars, n * sizeof(u256), hipMemcpyHostToDevice, ctx->stream));
  if (int32_t rc = scale_each_device<C>(ctx, d_pts.get(), n, d_k.get(), flags == G16_SCALARS_MONT, d_pts.get())) return rc;
  HIPCHK(ctx, hipMemcpyAsync(out, d_pts.get(), n * sizeof(typename C::Aff), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return G16_OK;
}

}  // namespace

extern "C" int32_t g16_points_scale_each_g1(g16_ctx* ctx, const void* points, size_t n, const void* scalars,
                                            uint32_t flags, void* out) {
  return points_scale_each<G1>(ctx, points, n, scalars, flags, out);
}
extern "C" int32_t g16_points_scale_each_g2(g16_ctx* ctx, const void* points, size_t n, const void* scalars,
                                            uint32_t flags, void* out) {
  return points_scale_each<G2>(ctx, points, n, scalars, flags, out);
}
extern "C" int32_t g16_points_scale_g1(g16_ctx* ctx, const void* points, size_t n, const void* k, uint32_t flags,
                                       void* out) {
  return points_scale<G1>(ctx, points, n, k, flags, out);
}
extern "C" int32_t g16_points_scale_g2(g16_ctx* ctx, const void* points, size_t n, const void* k, uint32_t flags,
                                       void* out) {
  return points_scale<G2>(ctx, points, n, k, flags, out);
}
