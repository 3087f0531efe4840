// Host logic of the MSM pipeline below the C ABI: the sort phase (shared by G1 and G2: it only looks at scalars) and
// the glue that strings the per-curve stages of an MSM together.  What is launched -- window, grids, workspaces, tail
// kernels -- is decided in msm_plan.hpp; the functions here build a plan once and launch what it says.  This translation
// unit holds the sort kernels only: the stage templates are declared in g16_internal.hpp and instantiated elsewhere.
#include "g16_internal.hpp"
#include "msm.cuh"

using namespace g16;

static_assert(MSM_FLAG_SCALARS_MONT == G16_SCALARS_MONT, "msm_plan.hpp and the C ABI disagree on the Montgomery flag");

// ---- phase 1: scalars -> bucket arrangement (count, scan, scatter, extra-segment list) ---------------------
int32_t g16_msm_sort(g16_ctx* ctx, hipStream_t st, const void* d_scalars, uint32_t flags, size_t n, uint32_t table_cfg,
                     g16_ctx::MsmSort& S, const uint32_t* d_live) {
  // everything the launches below depend on is decided here, once (msm_plan.hpp)
  const G16Env& env = g16_env();
  const MsmParams P = msm_params(n, flags, table_cfg, env);
  const MsmSortPlan L = msm_sort_plan(P, env);
  S.P = P;
  Carver measure{nullptr}, bind{nullptr};
  msm_sort_layout(S, P, L, measure);
  if (int32_t rc = ensure(ctx, S.buf, measure.bytes)) return rc;
  bind.base = (char*)S.buf.p();
  msm_sort_layout(S, P, L, bind);
  const auto* scalars = (const u256*)d_scalars;
  if (!L.use_part) HIPCHK(ctx, hipMemsetAsync(S.count, 0, (char*)S.offset - (char*)S.count, st));  // count + cursor are adjacent
  HIPCHK(ctx, hipMemsetAsync(S.info, 0, 64, st));
  HIPCHK(ctx, hipMemsetAsync(S.ghist, 0, PERM_BINS * 4, st));
  // a lean set (tables at a stride >= 2) runs the instantiations that map a window to its (table, bucket set) pair; every
  // other MSM the ones without that division
  const bool lean = P.tstride >= 2;
  if (L.use_part) {
    if (lean)
      KLAUNCH_ON(ctx, st, "msm_part_count", (part_pass<false, true>), L.ptiles, PART_BLOCK, 0, scalars, d_live, P, L.lo_bits,
                 L.nparts, L.ptiles, S.tile_hist, S.tmp);
    else
      KLAUNCH_ON(ctx, st, "msm_part_count", (part_pass<false, false>), L.ptiles, PART_BLOCK, 0, scalars, d_live, P, L.lo_bits,
                 L.nparts, L.ptiles, S.tile_hist, S.tmp);
    KLAUNCH_ON(ctx, st, "msm_scan", scan1_tile_sums, L.nt2, SCAN_BLOCK, 0, S.tile_hist, (uint32_t)L.nth, S.tiles2);
    KLAUNCH_ON(ctx, st, "msm_scan", scan_tiles, 1, SCAN_BLOCK, 0, S.tiles2, L.nt2, S.info + 8);  // total -> info[8]
    KLAUNCH_ON(ctx, st, "msm_scan", scan1_apply, L.nt2, SCAN_BLOCK, 0, S.tile_hist, (uint32_t)L.nth, S.tiles2);
    if (lean)
      KLAUNCH_ON(ctx, st, "msm_part_scatter", (part_pass<true, true>), L.ptiles, PART_BLOCK, 0, scalars, d_live, P, L.lo_bits,
                 L.nparts, L.ptiles, S.tile_hist, S.tmp);
    else
      KLAUNCH_ON(ctx, st, "msm_part_scatter", (part_pass<true, false>), L.ptiles, PART_BLOCK, 0, scalars, d_live, P, L.lo_bits,
                 L.nparts, L.ptiles, S.tile_hist, S.tmp);
    KLAUNCH_ON(ctx, st, "msm_bucket_sort", bucket_hist, L.nparts * BS_SPLIT, BS_LOW, 0, S.tmp, S.tile_hist, L.ptiles,
               L.nparts, S.info + 8, S.slice_hist);
    KLAUNCH_ON(ctx, st, "msm_bucket_sort", bucket_place, L.nparts * BS_SPLIT, BS_LOW, 0, S.tmp, S.tile_hist, L.ptiles,
               L.nparts, S.info + 8, S.slice_hist, P, L.lo_bits, S.count, S.offset, S.entries, L.fused ? 1u : 0u, S.xoff,
               S.heavy, S.info, S.ghist, S.blk_base);
  } else {
    if (lean)
      KLAUNCH_ON(ctx, st, "msm_count", msm_count<true>, L.nblk, MSM_BLOCK, 0, scalars, d_live, P, S.count);
    else
      KLAUNCH_ON(ctx, st, "msm_count", msm_count<false>, L.nblk, MSM_BLOCK, 0, scalars, d_live, P, S.count);
  }
  if (!L.fused) {
    KLAUNCH_ON(ctx, st, "msm_scan", scan_tile_sums, L.ntiles, SCAN_BLOCK, 0, S.count, P.nbuckets, P.seg, S.tiles);
    KLAUNCH_ON(ctx, st, "msm_scan", scan_tiles, 1, SCAN_BLOCK, 0, S.tiles, L.ntiles, S.info);
    KLAUNCH_ON(ctx, st, "msm_scan", scan_apply, L.ntiles, SCAN_BLOCK, 0, S.count, P.nbuckets, P.seg, S.tiles, S.offset,
               S.xoff, S.heavy, S.info);
    KLAUNCH_ON(ctx, st, "msm_perm", perm_hist, L.pblk, PERM_BLOCK, 0, S.count, P.nbuckets, S.ghist, S.blk_base);
  }
  KLAUNCH_ON(ctx, st, "msm_perm", perm_scatter, L.pblk, PERM_BLOCK, 0, S.count, P.nbuckets, S.ghist, S.blk_base,
             S.perm);
  if (!L.use_part) {
    if (lean)
      KLAUNCH_ON(ctx, st, "msm_scatter", msm_scatter<true>, L.nblk, MSM_BLOCK, 0, scalars, d_live, P, S.offset, S.cursor,
                 S.entries);
    else
      KLAUNCH_ON(ctx, st, "msm_scatter", msm_scatter<false>, L.nblk, MSM_BLOCK, 0, scalars, d_live, P, S.offset, S.cursor,
                 S.entries);
  }
  KLAUNCH_ON(ctx, st, "msm_make_extra", msm_make_extra, 512, MSM_BLOCK, 0, S.heavy, S.info, S.offset, S.xoff, P.seg,
             P.max_extra, S.xseg);
  HIPCHK(ctx, hipGetLastError());
  return G16_OK;
}

// phase 2: accumulate + reduce point sets against their bucket arrangements, `n_accum` jobs per launch (see
// g16_internal.hpp).
template <class C>
static int32_t msm_batch(g16_ctx* ctx, hipStream_t st, const g16_msm_run* runs, int n_accum, int n_tail,
                         hipEvent_t after_heavy) {
  if (n_accum < 1 || n_accum > MSM_BATCH_MAX || n_tail < 0 || n_tail > n_accum) {
    ctx->err = "bad MSM batch";
    return G16_EINVAL;
  }
  const MsmParams& P = runs[0].sort->P;
  constexpr size_t asz = sizeof(typename C::Acc);             // standard XYZZ (chunk sums and later): 128 / 256 B
  constexpr size_t psz29 = sizeof(typename Ec29<C>::Acc);     // reduced-radix XYZZ (bucket sums): 144 / 288 B
  static_assert(asz == 2 * sizeof(typename C::Aff) && psz29 * 8 == asz * 9, "accumulator sizes");   // 9 limbs for 8
  // workspace of a job: msm_job_layout, over the chunk count of the tail plan
  const MsmTailPlan T = msm_tail_plan(P, sizeof(typename C::Aff) == 64, runs[0].sort->narrow_tail, g16_env());
  MsmBatch<C> B;
  memset(&B, 0, sizeof B);
  Carver measure{nullptr};
  msm_job_layout(B.job[0], P, T.nchunks, asz, psz29, measure);
  for (int j = 0; j < n_accum; ++j) {
    const g16_ctx::MsmSort& S = *runs[j].sort;
    const MsmParams& Q = S.P;
    if (Q.n != P.n || Q.c != P.c || Q.nwin != P.nwin || Q.nbuckets != P.nbuckets || Q.seg != P.seg ||
        Q.tables != P.tables || Q.mtab != P.mtab || Q.tstride != P.tstride || Q.max_extra != P.max_extra) {
      ctx->err = "MSM batch: the jobs do not share their launch parameters";
      return G16_EINVAL;
    }
    if (int32_t rc = ensure(ctx, *runs[j].acc, measure.bytes)) return rc;
    MsmJob<C>& J = B.job[j];
    Carver bind{(char*)runs[j].acc->p()};
    msm_job_layout(J, P, T.nchunks, asz, psz29, bind);
    J.points = (const typename Ec29<C>::Tab*)runs[j].d_points;
    J.entries = S.entries;
    J.offset = S.offset;
    J.xseg = S.xseg;
    J.info = S.info;
    J.perm = S.perm;
    J.heavy = S.heavy;
    J.xoff = S.xoff;
    J.init = (const typename Ec29<C>::Acc*)runs[j].init_partial;
    J.out_aff = (typename C::Aff*)runs[j].d_out_aff;
    J.out_acc = (typename C::Acc*)runs[j].d_out_acc;
    if (runs[j].sparse) {
      // the job read no arrangement: no extra segment and no split bucket (zero counters), slot = bucket, every bucket
      // written -- a view of its own, so that nothing of the tail looks into the sort the other jobs share
      J.entries = J.offset = J.perm = J.heavy = J.xoff = nullptr;
      J.xseg = nullptr;
      J.info = runs[j].sparse->d_info;
    }
  }
  // the accumulate stage: msm_accum over the jobs that run against their arrangement -- the batch without the sparse
  // ones, in order -- and the sparse run of each of the others.  One profile entry for the stage either way.
  MsmBatch<C> D = B;
  int n_dense = 0;
  for (int j = 0; j < n_accum; ++j)
    if (!runs[j].sparse) D.job[n_dense++] = B.job[j];
  int32_t rc;
  if (n_dense && (rc = stage_accum<C>(ctx, st, P, D, n_dense))) return rc;
  bool listed = n_dense != 0;
  for (int j = 0; j < n_accum; ++j) {
    if (!runs[j].sparse) continue;
    if constexpr (sizeof(typename C::Aff) == 64) {
      if ((rc = stage_accum_sparse<C>(ctx, st, P, *runs[j].sparse, runs[j].d_points, B.job[j].partial, !listed))) return rc;
      listed = true;
    }
  }
  if ((rc = stage_heavy<C>(ctx, st, P, T, B, n_accum))) return rc;
  if (after_heavy) HIPCHK(ctx, hipEventRecord(after_heavy, st));
  if (!n_tail) return G16_OK;
  if ((rc = stage_reduce1<C>(ctx, st, P, T, B, n_tail))) return rc;
  return stage_reduce2_fold<C>(ctx, st, P, T, B, n_tail);
}
int32_t g16_msm_batch(g16_ctx* ctx, hipStream_t stream, int group, const g16_msm_run* runs, int n_accum, int n_tail,
                      hipEvent_t after_heavy) {
  // a null table stands for a set at infinity throughout, and msm_accum then drops the sums it was given to continue
  for (int i = 0; i < n_accum; ++i)
    if (!runs[i].d_points && runs[i].init_partial) {
      ctx->err = "an MSM run without a table cannot continue another run's bucket sums";
      return G16_EINVAL;
    }
  // the sparse run is G1's, gathers from a table and starts every bucket from infinity
  for (int i = 0; i < n_accum; ++i)
    if (runs[i].sparse && (group != 1 || !runs[i].d_points || runs[i].init_partial || !runs[i].sparse->d_wires ||
                           !runs[i].sparse->d_info || !runs[i].sparse->d_scalars)) {
      ctx->err = "a sparse MSM run needs a G1 table, its scalars and wire list, and continues no other run";
      return G16_EINVAL;
    }
  return group == 1 ? msm_batch<G1>(ctx, stream, runs, n_accum, n_tail, after_heavy)
                    : msm_batch<G2>(ctx, stream, runs, n_accum, n_tail, after_heavy);
}

// one complete MSM on the context's main stream
template <class C>
int32_t msm_device(g16_ctx* ctx, const void* d_scalars, uint32_t flags, const void* d_points, size_t n, void* d_out_aff,
                   void* d_out_acc, uint32_t table_c, const uint32_t* d_live) {
  ctx->sort[0].narrow_tail = false;   // stand-alone MSM: nothing overlaps its tail, the short chain wins
  int32_t rc = g16_msm_sort(ctx, ctx->stream, d_scalars, flags, n, table_c, ctx->sort[0], d_live);
  if (rc) return rc;
  if ((table_c & 0xffu) == 0 && n) {   // plain point array: the accumulate kernel reads reduced-radix entries
    static_assert(sizeof(typename Ec29<C>::Tab) == sizeof(typename C::Aff), "packed entries: 64 / 128 B");
    if ((rc = ensure(ctx, ctx->stage_p29, n * sizeof(typename Ec29<C>::Tab)))) return rc;
    if ((rc = to29_device<C>(ctx, ctx->stream, d_points, n, ctx->stage_p29.p()))) return rc;
    d_points = ctx->stage_p29.p();
  }
  const g16_msm_run run{&ctx->sort[0], &ctx->lane[0].acc, d_points, d_out_aff, d_out_acc, nullptr};
  return msm_batch<C>(ctx, ctx->stream, &run, 1, 1, nullptr);
}
template int32_t msm_device<G1>(g16_ctx*, const void*, uint32_t, const void*, size_t, void*, void*, uint32_t, const uint32_t*);
template int32_t msm_device<G2>(g16_ctx*, const void*, uint32_t, const void*, size_t, void*, void*, uint32_t, const uint32_t*);
