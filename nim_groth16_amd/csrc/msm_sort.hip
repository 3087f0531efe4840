// Host logic of the MSM pipeline below the C ABI: window choice, launch parameters, the sort phase (shared by G1 and
// G2: it only looks at scalars) and the glue that strings the per-curve stages of an MSM together.  This translation
// unit holds the sort kernels only: the stage templates are declared in g16_internal.hpp and instantiated elsewhere.
#include "g16_internal.hpp"
#include "msm.cuh"

using namespace g16;

// Window size by a cost model: accumulation = n * nwin mixed adds (~10 modmul each); bucket reduction =
// 2 XYZZ adds (~14 modmul each) per bucket, over nwin bucket sets -- or over ONE set when the points come
// with precomputed 2^(c w) tables (`merged`).  A short top window (t = 254 - (nwin-1) c bits) would map all n
// scalars onto 2^t buckets, so candidates need t >= min(c-2, 6).  2^20 points: c = 16 plain, c = 20 merged
// (13 tables instead of 16 windows).
static uint32_t pick_window_cost(size_t n, bool merged, int forced, uint32_t cmax) {
  if (forced) return (uint32_t)forced;   // G16_MSM_WINDOW / G16_TABLE_WINDOW (g16_env: read once per process)
  uint32_t best = 5;
  double best_cost = 1e300;
  for (uint32_t c = 5; c <= cmax; ++c) {
    const uint32_t nwin = FR_BITS / c + 1;
    if (((size_t)nwin * n) >> 31) continue;   // table index / entry count must fit 31 bits
    const uint32_t t = FR_BITS - (nwin - 1) * c, tmin = c - 2 < 6 ? c - 2 : 6;
    if (t < tmin && c > 5) continue;
    const double sets = merged ? 1.0 : (double)nwin;
    const double cost = 10.0 * (double)n * nwin + 28.0 * sets * (double)(1u << (c - 1));
    if (cost < best_cost) {
      best_cost = cost;
      best = c;
    }
  }
  return best;
}
static uint32_t pick_window(size_t n) { return pick_window_cost(n ? n : 1, false, g16_env().msm_window, 16); }

// table_cfg: 0 for a plain point array, else the window bits of a registered set | its multiplier tables << 8
// (g16_points::cfg)
static MsmParams msm_params(size_t n, uint32_t flags, uint32_t table_cfg) {
  MsmParams P;
  const uint32_t table_c = table_cfg & 0xffu;
  P.n = (uint32_t)n;
  P.c = table_c ? table_c : pick_window(n);
  P.nwin = FR_BITS / P.c + 1;
  P.tables = table_c ? 1u : 0u;
  P.mtab = table_c && (table_cfg >> 8) == 2 ? 2u : 1u;
  P.nbuckets = P.tables ? msm_table_buckets(P.c, P.mtab) : (P.nwin << (P.c - 1));
  // segment length L: one accumulate task handles <= L entries.  A task is a serial chain of L mixed adds
  // (~23 us each with 4 waves per SIMD), so L also bounds the tail of the launch; ~1.25 x the mean bucket size
  // keeps most buckets in one segment, the rest get 1-2 short extra segments that msm_reduce1 absorbs.
  // (class bucket set: a bucket serves one or two digit values -- size the segment for the two-value buckets, or most
  // of them are split: 112 instead of 121 proofs/s, profiles/r04_ab_mtab_seg.txt)
  size_t avg = P.mtab == 2 ? ((size_t)n * P.nwin * 2) / (size_t(1) << (P.c - 1)) + 1 : ((size_t)n * P.nwin) / P.nbuckets + 1;
  P.seg = (uint32_t)(((avg + avg / 4 + 15) / 16) * 16);
  // few, long buckets (small windows / small point sets): cut them so that the launch still has ~64 k tasks --
  // a task is a serial chain, and 2^11 buckets of 1500 entries each would otherwise run as 2^11 threads
  const size_t cap = (((size_t)n * P.nwin / 65536 + 15) / 16) * 16;
  if (P.seg > cap) P.seg = (uint32_t)cap;
  if (P.seg < 32) P.seg = 32;
  if (g16_env().msm_seg) P.seg = (uint32_t)g16_env().msm_seg;
  P.scalars_mont = (flags & G16_SCALARS_MONT) ? 1u : 0u;
  P.max_extra = (uint32_t)(((size_t)P.n * P.nwin) / P.seg + 1);
  return P;
}

uint32_t g16_pick_table_window(size_t n) { return pick_window_cost(n ? n : 1, true, g16_env().table_window, 22); }
// multiplier tables of a registered set with window c: the 43 slices of 2^(c-7) buckets of the class bucket set must
// be whole 256-bucket partitions of the sort
uint32_t g16_pick_mtab(uint32_t c) { return g16_env().mtab == 2 && c >= 15 ? 2u : 1u; }

// A workspace is cut from one buffer, part after part, each rounded up to 256 bytes.  Its layout is written once, as a
// function that names the pointer and the size of every part in order, and run twice: without a base, to add up the
// bytes that ensure() has to provide, and then over the buffer, to point the parts into it.
struct Carver {
  char* base;
  size_t bytes = 0;
  template <class T>
  void operator()(T*& part, size_t size) {
    if (base) part = (T*)(base + bytes);
    bytes += (size + 255) & ~size_t(255);
  }
};

// ---- phase 1: scalars -> bucket arrangement (count, scan, scatter, extra-segment list) ---------------------
int32_t g16_msm_sort(g16_ctx* ctx, hipStream_t st, const void* d_scalars, uint32_t flags, size_t n, uint32_t table_cfg,
                     g16_ctx::MsmSort& S, const uint32_t* d_live) {
  const MsmParams P = msm_params(n, flags, table_cfg);
  S.P = P;
  // partition sort (see msm.cuh): low bits <= BS_LOG (as many as divide the bucket count: the class set of a
  // registered set is 43 * 2^(c-7) buckets), partitions = nwin << hi_bits
  uint32_t lo_bits = P.c - 1 < (uint32_t)BS_LOG ? P.c - 1 : (uint32_t)BS_LOG;
  while (lo_bits && (P.nbuckets & ((1u << lo_bits) - 1))) --lo_bits;
  const uint32_t nparts = P.nbuckets >> lo_bits;
  const uint32_t ptiles = (P.n + PART_TILE - 1) / PART_TILE;
  const bool use_part = nparts <= PART_MAX && g16_env().msm_sort != 'a';
  const size_t nth = (size_t)nparts * ptiles;
  const size_t nb = P.nbuckets;
  auto layout = [&](Carver& part) {
    part(S.count, nb * 4);   // count + cursor are adjacent: one memset clears both
    part(S.cursor, nb * 4);
    part(S.offset, (nb + 1) * 4);
    part(S.xoff, nb * 4);
    part(S.heavy, nb * 4);
    part(S.info, 64);
    part(S.tiles, ((nb + SCAN_TILE - 1) / SCAN_TILE) * 8);
    part(S.entries, (size_t)P.n * P.nwin * 4);
    part(S.xseg, (size_t)P.max_extra * 8);
    part(S.perm, nb * 4);
    part(S.ghist, PERM_BINS * 4);
    part(S.blk_base, ((nb + PERM_BLOCK - 1) / PERM_BLOCK) * PERM_BINS * 4);
    part(S.tile_hist, use_part ? nth * 4 : 4);
    part(S.tmp, use_part ? (size_t)P.n * P.nwin * 8 : 8);
    part(S.tiles2, ((nth + SCAN_TILE - 1) / SCAN_TILE) * 8 + 8);
    part(S.slice_hist, use_part ? (size_t)nparts * BS_SPLIT * BS_LOW * 4 : 4);
  };
  Carver measure{nullptr}, bind{nullptr};
  layout(measure);
  if (int32_t rc = ensure(ctx, S.buf, measure.bytes)) return rc;
  bind.base = (char*)S.buf.p();
  layout(bind);
  const auto* scalars = (const u256*)d_scalars;
  // lo_bits == BS_LOG: bucket_place also produces xoff / heavy / the size histogram (see msm.cuh); count[] and
  // offset[] are fully written by it, so the partition path clears only the two small counter blocks
  const bool fused = use_part && lo_bits == (uint32_t)BS_LOG;
  if (!use_part) HIPCHK(ctx, hipMemsetAsync(S.count, 0, (char*)S.offset - (char*)S.count, st));  // count + cursor are adjacent
  HIPCHK(ctx, hipMemsetAsync(S.info, 0, 64, st));
  HIPCHK(ctx, hipMemsetAsync(S.ghist, 0, PERM_BINS * 4, st));
  const uint32_t nblk = (P.n + MSM_BLOCK - 1) / MSM_BLOCK;
  const uint32_t ntiles = (P.nbuckets + SCAN_TILE - 1) / SCAN_TILE;
  if (use_part) {
    const uint32_t nt2 = (uint32_t)((nth + SCAN_TILE - 1) / SCAN_TILE);
    KLAUNCH_ON(ctx, st, "msm_part_count", part_pass<false>, ptiles, PART_BLOCK, 0, scalars, d_live, P, lo_bits, nparts, ptiles,
               S.tile_hist, S.tmp);
    KLAUNCH_ON(ctx, st, "msm_scan", scan1_tile_sums, nt2, SCAN_BLOCK, 0, S.tile_hist, (uint32_t)nth, S.tiles2);
    KLAUNCH_ON(ctx, st, "msm_scan", scan_tiles, 1, SCAN_BLOCK, 0, S.tiles2, nt2, S.info + 8);  // total -> info[8]
    KLAUNCH_ON(ctx, st, "msm_scan", scan1_apply, nt2, SCAN_BLOCK, 0, S.tile_hist, (uint32_t)nth, S.tiles2);
    KLAUNCH_ON(ctx, st, "msm_part_scatter", part_pass<true>, ptiles, PART_BLOCK, 0, scalars, d_live, P, lo_bits, nparts,
               ptiles, S.tile_hist, S.tmp);
    KLAUNCH_ON(ctx, st, "msm_bucket_sort", bucket_hist, nparts * BS_SPLIT, BS_LOW, 0, S.tmp, S.tile_hist, ptiles, nparts,
               S.info + 8, S.slice_hist);
    KLAUNCH_ON(ctx, st, "msm_bucket_sort", bucket_place, nparts * BS_SPLIT, BS_LOW, 0, S.tmp, S.tile_hist, ptiles, nparts,
               S.info + 8, S.slice_hist, P, lo_bits, S.count, S.offset, S.entries, fused ? 1u : 0u, S.xoff, S.heavy,
               S.info, S.ghist, S.blk_base);
  } else {
    KLAUNCH_ON(ctx, st, "msm_count", msm_count, nblk, MSM_BLOCK, 0, scalars, d_live, P, S.count);
  }
  const uint32_t pblk = (P.nbuckets + PERM_BLOCK - 1) / PERM_BLOCK;
  if (!fused) {
    KLAUNCH_ON(ctx, st, "msm_scan", scan_tile_sums, ntiles, SCAN_BLOCK, 0, S.count, P.nbuckets, P.seg, S.tiles);
    KLAUNCH_ON(ctx, st, "msm_scan", scan_tiles, 1, SCAN_BLOCK, 0, S.tiles, ntiles, S.info);
    KLAUNCH_ON(ctx, st, "msm_scan", scan_apply, ntiles, SCAN_BLOCK, 0, S.count, P.nbuckets, P.seg, S.tiles, S.offset,
               S.xoff, S.heavy, S.info);
    KLAUNCH_ON(ctx, st, "msm_perm", perm_hist, pblk, PERM_BLOCK, 0, S.count, P.nbuckets, S.ghist, S.blk_base);
  }
  KLAUNCH_ON(ctx, st, "msm_perm", perm_scatter, pblk, PERM_BLOCK, 0, S.count, P.nbuckets, S.ghist, S.blk_base,
             S.perm);
  if (!use_part)
    KLAUNCH_ON(ctx, st, "msm_scatter", msm_scatter, nblk, MSM_BLOCK, 0, scalars, d_live, P, S.offset, S.cursor, S.entries);
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
  const size_t nchunks = P.nbuckets / msm_red_chunk(P);
  // workspace of a job (the bucket sums come first: g16_msm_partial_ptr)
  auto layout = [&](MsmJob<C>& J, Carver& part) {
    part(J.partial, ((size_t)P.nbuckets + P.max_extra) * psz29);
    part(J.chunkR, nchunks * asz);
    part(J.chunkA, nchunks * asz);
    part(J.wsum, (size_t)(2 * 64 + 2) * asz);
  };
  MsmBatch<C> B;
  memset(&B, 0, sizeof B);
  Carver measure{nullptr};
  layout(B.job[0], measure);
  for (int j = 0; j < n_accum; ++j) {
    const g16_ctx::MsmSort& S = *runs[j].sort;
    const MsmParams& Q = S.P;
    if (Q.n != P.n || Q.c != P.c || Q.nwin != P.nwin || Q.nbuckets != P.nbuckets || Q.seg != P.seg ||
        Q.tables != P.tables || Q.mtab != P.mtab || Q.max_extra != P.max_extra) {
      ctx->err = "MSM batch: the jobs do not share their launch parameters";
      return G16_EINVAL;
    }
    if (int32_t rc = ensure(ctx, *runs[j].acc, measure.bytes)) return rc;
    MsmJob<C>& J = B.job[j];
    Carver bind{(char*)runs[j].acc->p()};
    layout(J, bind);
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
  }
  int32_t rc;
  if ((rc = stage_accum<C>(ctx, st, P, B, n_accum))) return rc;
  if ((rc = stage_heavy<C>(ctx, st, P, B, n_accum))) return rc;
  if (after_heavy) HIPCHK(ctx, hipEventRecord(after_heavy, st));
  if (!n_tail) return G16_OK;
  if ((rc = stage_reduce1<C>(ctx, st, P, B, n_tail))) return rc;
  return stage_reduce2_fold<C>(ctx, st, P, runs[0].sort->narrow_tail, B, n_tail);
}
int32_t g16_msm_batch(g16_ctx* ctx, hipStream_t stream, int group, const g16_msm_run* runs, int n_accum, int n_tail,
                      hipEvent_t after_heavy) {
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
