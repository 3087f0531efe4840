// Bodies of the per-curve launch templates that g16_internal.hpp declares: the accumulate / reduce stages and the
// auxiliary point kernels.  Included only by msm_g1_*.hip and msm_g2_*.hip, each of which explicitly instantiates its
// share for one curve: the fully inlined G2 kernels take minutes to compile, and `make -j` builds the stages in
// parallel.  Every other translation unit calls the templates through their declarations and instantiates no kernel.
#pragma once
#include "g16_internal.hpp"
#include "msm.cuh"

using namespace g16;

// B: `ny` jobs that share the launch parameters P (same n, same window: the G1 MSMs of a proof)
template <class C>
int32_t stage_accum(g16_ctx* ctx, hipStream_t st, const MsmParams& P, const MsmBatch<C>& B, uint32_t ny) {
  const bool g2 = sizeof(typename C::Aff) == 128;
  const uint32_t ntask = P.nbuckets + P.max_extra;
  KLAUNCH_ON(ctx, st, g2 ? "msm_accum_g2" : "msm_accum_g1", msm_accum<C>, dim3((ntask + ACC_BLOCK - 1) / ACC_BLOCK, ny),
             ACC_BLOCK, 0, B, P, ctx->profiling ? ctx->clk_buf.get() : (unsigned long long*)nullptr);
  HIPCHK(ctx, hipGetLastError());
  return G16_OK;
}

// The sparse run of one job: the same grid over the bucket slots as msm_accum's, without the extra segments -- the run has
// none.  Under the profile name of the accumulate stage it stands for (one launch of a proof, as ever).
template <class C>
int32_t stage_accum_sparse(g16_ctx* ctx, hipStream_t st, const MsmParams& P, const g16_msm_sparse& sp, const void* d_points,
                           void* d_partial, bool own_entry) {
  static_assert(sizeof(typename C::Aff) == 64, "the sparse run is instantiated for G1");
  const dim3 grid((P.nbuckets + ACC_BLOCK - 1) / ACC_BLOCK);
  const auto* points = (const typename Ec29<C>::Tab*)d_points;
  auto* partial = (typename Ec29<C>::Acc*)d_partial;
  if (own_entry)
    KLAUNCH_ON(ctx, st, "msm_accum_g1", msm_sparse_accum<C>, grid, ACC_BLOCK, 0, points, (const u256*)sp.d_scalars, sp.d_wires,
               sp.nlive, P, partial);
  else
    hipLaunchKernelGGL(msm_sparse_accum<C>, grid, dim3(ACC_BLOCK), 0, st, points, (const u256*)sp.d_scalars, sp.d_wires,
                       sp.nlive, P, partial);
  HIPCHK(ctx, hipGetLastError());
  return G16_OK;
}

template <class C>
int32_t stage_heavy(g16_ctx* ctx, hipStream_t st, const MsmParams& P, const MsmTailPlan& T, const MsmBatch<C>& B,
                    uint32_t ny) {
  const bool g2 = sizeof(typename C::Aff) == 128;
  KLAUNCH_ON(ctx, st, g2 ? "msm_heavy_g2" : "msm_heavy_g1", msm_heavy<C>, dim3(T.heavy_grid(ny), ny), heavy_block<C>(),
             heavy_block<C>() * sizeof(typename Ec29<C>::Acc), B, P);
  HIPCHK(ctx, hipGetLastError());
  return G16_OK;
}

template <class C>
int32_t stage_reduce1(g16_ctx* ctx, hipStream_t st, const MsmParams& P, const MsmTailPlan& T, const MsmBatch<C>& B,
                      uint32_t ny) {
  const bool g2 = sizeof(typename C::Aff) == 128;
  KLAUNCH_ON(ctx, st, g2 ? "msm_reduce1_g2" : "msm_reduce1_g1", msm_reduce1<C>,
             dim3((uint32_t)((T.nchunks + MSM_BLOCK - 1) / MSM_BLOCK), ny), MSM_BLOCK, 0, B, P.nbuckets, T.rc);
  HIPCHK(ctx, hipGetLastError());
  return G16_OK;
}

// MsmJob::wsum: room for 2 * 64 + 2 accumulators
// Which reduce2 and which fold, over which slices: msm_tail_plan (msm_plan.hpp).  One launch per kernel variant.
template <class C>
int32_t stage_reduce2_fold(g16_ctx* ctx, hipStream_t st, const MsmParams& P, const MsmTailPlan& T, const MsmBatch<C>& B,
                           uint32_t ny) {
  const bool g2 = sizeof(typename C::Aff) == 128;
  constexpr bool is_g1 = sizeof(typename C::Aff) == 64;
  constexpr int R2B = is_g1 ? 512 : 256;   // MsmR2::WIDE; NARROW is a quarter of it
  constexpr int R2N = R2B / 4;
  const char* nm = g2 ? "msm_reduce2_g2" : "msm_reduce2_g1";
  const dim3 grid(T.nsets, ny);
  const size_t lds = T.r2_lds * sizeof(typename C::Acc);
  switch (T.r2) {
    case MsmR2::QUAD128:
      KLAUNCH_ON(ctx, st, nm, (msm_reduce2<C, Quad<C>, is_g1 ? 128 : 64>), grid, T.r2_threads, lds, B, T.cps, T.rc);
      break;
    case MsmR2::QUAD64:
      KLAUNCH_ON(ctx, st, nm, (msm_reduce2<C, Quad<C>, 64>), grid, T.r2_threads, lds, B, T.cps, T.rc);
      break;
    case MsmR2::WIDE:
      KLAUNCH_ON(ctx, st, nm, (msm_reduce2<C, Lane<C>, R2B>), grid, T.r2_threads, lds, B, T.cps, T.rc);
      break;
    case MsmR2::WAVE:
      KLAUNCH_ON(ctx, st, nm, (msm_reduce2<C, Lane<C>, 64>), grid, T.r2_threads, lds, B, T.cps, T.rc);
      break;
    case MsmR2::NARROW:
      KLAUNCH_ON(ctx, st, nm, (msm_reduce2<C, Lane<C>, R2N>), grid, T.r2_threads, lds, B, T.cps, T.rc);
      break;
  }
  nm = g2 ? "msm_fold_g2" : "msm_fold_g1";
  switch (T.fold) {
    case MsmFold::CLASSES_QUAD:
      KLAUNCH_ON(ctx, st, nm, msm_fold_classes_quad<C>, dim3(1, ny), 512, 128 * sizeof(typename C::Acc), B, T.log2ks);
      break;
    case MsmFold::CLASSES:
      KLAUNCH_ON(ctx, st, nm, msm_fold_classes<C>, dim3(1, ny), 128, 0, B, T.log2ks);
      break;
    case MsmFold::MERGED:
      KLAUNCH_ON(ctx, st, nm, msm_fold_merged<C>, dim3(1, ny), 128, 0, B, T.nsets, T.log2ks);
      break;
    case MsmFold::PLAIN:
      KLAUNCH_ON(ctx, st, nm, msm_fold<C>, dim3(1, ny), 64, 0, B, T.nsets, P.c);
      break;
  }
  HIPCHK(ctx, hipGetLastError());
  return G16_OK;
}

// sum of XYZZ partials -> affine (the `res += sync pending[k]` of msm.nim:117-119 across GPUs)
template <class C>
__global__ void sum_partials_kernel(const typename C::Acc* __restrict__ parts, uint32_t count,
                                    typename C::Aff* __restrict__ out) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  typename C::Acc r = C::acc_inf();
  for (uint32_t i = 0; i < count; ++i) C::add(r, parts[i]);
  *out = C::to_affine(r);
}

template <class C>
int32_t sum_partials_device(g16_ctx* ctx, const void* d_parts, uint32_t count, void* d_out_aff) {
  KLAUNCH(ctx, "sum_partials", sum_partials_kernel<C>, 1, 64, 0, (const typename C::Acc*)d_parts, count,
          (typename C::Aff*)d_out_aff);
  HIPCHK(ctx, hipGetLastError());
  return G16_OK;
}

// stride: tables for every stride-th window (1: every window; >= 2: a lean set, mtab == 1)
template <class C>
int32_t precompute_device(g16_ctx* ctx, const void* d_points, size_t n, uint32_t c, uint32_t mtab, uint32_t stride,
                          void* d_tables) {
  const uint32_t nwin = FR_BITS / c + 1, ntab = (nwin + stride - 1) / stride;
  KLAUNCH(ctx, "msm_precompute", msm_precompute<C>, (uint32_t)((n + MSM_BLOCK - 1) / MSM_BLOCK), MSM_BLOCK, 0,
          (const typename C::Aff*)d_points, (uint32_t)n, c * stride, ntab, mtab, (typename Ec29<C>::Tab*)d_tables);
  HIPCHK(ctx, hipGetLastError());
  return G16_OK;
}

// reference-layout points -> reduced-radix entries (the one-shot MSM entry points, which have no tables)
template <class C>
int32_t to29_device(g16_ctx* ctx, hipStream_t st, const void* d_points, size_t n, void* d_out) {
  if (n)
    KLAUNCH_ON(ctx, st, "points_to29", points_to29<C>, (uint32_t)((n + MSM_BLOCK - 1) / MSM_BLOCK), MSM_BLOCK, 0,
               (const typename C::Aff*)d_points, (uint32_t)n, (typename Ec29<C>::Tab*)d_out);
  HIPCHK(ctx, hipGetLastError());
  return G16_OK;
}

// Curve constants in Montgomery form, specialised beside the instantiations that use them (msm_g{1,2}_misc.hip):
//   static typename C::Aff gen();   the group generator
//   static typename C::E b();       the constant of y^2 = x^3 + b
template <class C>
struct CurveConsts;

// d_table: 32*255 multiples of the generator (built here when !table_ready)
template <class C>
int32_t fixed_base_device(g16_ctx* ctx, void* d_table, bool table_ready, const void* d_scalars, uint32_t mont, size_t n,
                          void* d_out) {
  if (!table_ready)
    KLAUNCH(ctx, "fixed_base_table", fixed_base_table<C>, (32 * 255 + 255) / 256, 256, 0, CurveConsts<C>::gen(),
            (typename C::Aff*)d_table);
  if (n)
    KLAUNCH(ctx, "fixed_base_mul", fixed_base_mul<C>, (uint32_t)((n + 255) / 256), 256, 0, (const u256*)d_scalars,
            mont, (uint32_t)n, (const typename C::Aff*)d_table, (typename C::Aff*)d_out);
  HIPCHK(ctx, hipGetLastError());
  return G16_OK;
}

// first_bad (device u32) must hold 0xffffffff on entry
template <class C>
int32_t on_curve_device(g16_ctx* ctx, const void* d_points, size_t n, uint32_t* d_first_bad) {
  if (n)
    KLAUNCH(ctx, "points_on_curve", points_on_curve<C>, (uint32_t)((n + 255) / 256), 256, 0,
            (const typename C::Aff*)d_points, (uint32_t)n, CurveConsts<C>::b(), d_first_bad);
  HIPCHK(ctx, hipGetLastError());
  return G16_OK;
}

template <class C>
int32_t live_bitmap_device(g16_ctx* ctx, const void* d_points, size_t n, uint32_t* d_bitmap, uint32_t* d_n_inf) {
  if (n)
    KLAUNCH(ctx, "points_live_bitmap", points_live_bitmap<C>, (uint32_t)((n + 255) / 256), 256, 0,
            (const typename C::Aff*)d_points, (uint32_t)n, d_bitmap, d_n_inf);
  HIPCHK(ctx, hipGetLastError());
  return G16_OK;
}
