// The launch plan of an MSM (msm_sort.hip, msm_stage.cuh), decided once: window and parameters, the grids of the sort,
// the two workspaces part by part, and which reduce2 / fold kernel forms the tail over which slices.  Everything here
// is a pure function of its arguments -- the knobs come in as a G16Env -- and plain C++: the CPU test shim builds it
// with g++ and holds every plan to a restated rule (tests/test_msm_plan_cpu.py), as it does for ntt_plan.hpp.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "g16_env.hpp"
#include "msm_params.hpp"

namespace g16 {

// ---- window and parameters ------------------------------------------------------------------------------------------
// Window size by a cost model: accumulation = n * nwin mixed adds (~10 modmul each); bucket reduction =
// 2 XYZZ adds (~14 modmul each) per bucket, over nwin bucket sets -- or over ONE set when the points come
// with precomputed 2^(c w) tables (`merged`).  A short top window (t = 254 - (nwin-1) c bits) would map all n
// scalars onto 2^t buckets, so candidates need t >= min(c-2, 6).  2^20 points: c = 16 plain, c = 20 merged
// (13 tables instead of 16 windows).
// `stride` >= 2 (a lean registered set, below): min(stride, nwin) bucket sets.
inline uint32_t msm_pick_window_cost(size_t n, bool merged, int forced, uint32_t cmax, uint32_t stride = 0) {
  if (forced) return (uint32_t)forced;   // G16_MSM_WINDOW / G16_TABLE_WINDOW
  uint32_t best = 5;
  double best_cost = 1e300;
  for (uint32_t c = 5; c <= cmax; ++c) {
    const uint32_t nwin = FR_BITS / c + 1;
    if (((size_t)nwin * n) >> 31) continue;   // table index / entry count must fit 31 bits
    const uint32_t t = FR_BITS - (nwin - 1) * c, tmin = c - 2 < 6 ? c - 2 : 6;
    if (t < tmin && c > 5) continue;
    const double sets = merged ? 1.0 : (double)(stride >= 2 && stride < nwin ? stride : nwin);
    const double cost = 10.0 * (double)n * nwin + 28.0 * sets * (double)(1u << (c - 1));
    if (cost < best_cost) {
      best_cost = cost;
      best = c;
    }
  }
  return best;
}
inline uint32_t msm_pick_window(size_t n, const G16Env& env) {
  return msm_pick_window_cost(n ? n : 1, false, env.msm_window, 16);
}
// window bits / multiplier tables of a registered set of n points
inline uint32_t msm_pick_table_window(size_t n, const G16Env& env) {
  return msm_pick_window_cost(n ? n : 1, true, env.table_window, 22);
}
// multiplier tables of a registered set with window c: the 43 slices of 2^(c-7) buckets of the class bucket set must
// be whole 256-bucket partitions of the sort
inline uint32_t msm_pick_mtab(uint32_t c, const G16Env& env) { return env.mtab == 2 && c >= 15 ? 2u : 1u; }
// Lean registered sets: tables at a stride.  Table j of a set registered at stride s holds 2^(c s j) P_i, and window
// w = s j + r gathers from table j into bucket set r (msm_window_slot): ceil(nwin / s) tables instead of nwin, s bucket
// sets of 2^(c-1) buckets instead of one.  A stride above nwin is nwin -- the one-shot layout with the points resident.
// The window comes from the same cost model over s bucket sets, capped like a one-shot MSM's: every bucket set the tail
// then sees has a shape that the one-shot path runs as well.
inline uint32_t msm_pick_lean_window(size_t n, uint32_t stride, const G16Env& env) {
  return msm_pick_window_cost(n ? n : 1, false, env.table_window, 16, stride);
}
inline uint32_t msm_clamp_stride(uint32_t stride, uint32_t c) {
  const uint32_t nwin = FR_BITS / c + 1;
  return stride > nwin ? nwin : stride;
}
// what registration decides for n points at a table stride (0 / 1: a table per window), before any fallback for lack of
// HBM: window bits, multiplier tables, the stride as it is used, and the tables that hold the set
struct MsmTableChoice {
  uint32_t c, mtab, stride, ntables;
  bool fits;   // table indices and entry counts stay below 2^31
};
inline MsmTableChoice msm_table_choice(size_t n, uint32_t stride, const G16Env& env) {
  MsmTableChoice t;
  if (stride >= 2) {
    t.c = msm_pick_lean_window(n, stride, env);
    t.mtab = 1;
    t.stride = msm_clamp_stride(stride, t.c);
  } else {
    t.c = msm_pick_table_window(n, env);
    t.mtab = msm_pick_mtab(t.c, env);
    t.stride = 1;
  }
  const uint32_t nwin = FR_BITS / t.c + 1;
  if ((size_t)t.mtab * nwin * n >= (size_t(1) << 31)) t.mtab = 1;
  t.ntables = t.mtab * ((nwin + t.stride - 1) / t.stride);
  t.fits = (size_t)nwin * n < (size_t(1) << 31);   // the entries; the table index ntables * n is no larger
  return t;
}
// table_cfg of a registered set (g16_points::cfg): window bits | multiplier tables << 8 | table stride << 16 (0 = 1)
inline uint32_t msm_table_cfg(uint32_t c, uint32_t mtab, uint32_t stride) {
  return c | (mtab << 8) | (stride >= 2 ? stride << 16 : 0u);
}

constexpr uint32_t MSM_FLAG_SCALARS_MONT = 1u;   // = G16_SCALARS_MONT of the C ABI (asserted in msm_sort.hip)

// table_cfg: 0 for a plain point array, else the window bits of a registered set | its multiplier tables << 8 | its
// table stride << 16 (g16_points::cfg, msm_table_cfg; a stride of 0 there is 1)
inline MsmParams msm_params(size_t n, uint32_t flags, uint32_t table_cfg, const G16Env& env) {
  MsmParams P;
  const uint32_t table_c = table_cfg & 0xffu;
  P.n = (uint32_t)n;
  P.c = table_c ? table_c : msm_pick_window(n, env);
  P.nwin = FR_BITS / P.c + 1;
  P.tables = table_c ? 1u : 0u;
  const uint32_t stride = table_c ? msm_clamp_stride(table_cfg >> 16, P.c) : 0u;
  P.tstride = table_c ? (stride >= 2 ? stride : 1u) : 0u;
  P.mtab = table_c && P.tstride == 1 && ((table_cfg >> 8) & 0xffu) == 2 ? 2u : 1u;
  P.nbuckets = P.tstride >= 2 ? (P.tstride << (P.c - 1)) : P.tables ? msm_table_buckets(P.c, P.mtab) : (P.nwin << (P.c - 1));
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
  if (env.msm_seg) P.seg = (uint32_t)env.msm_seg;
  P.scalars_mont = (flags & MSM_FLAG_SCALARS_MONT) ? 1u : 0u;
  P.max_extra = (uint32_t)(((size_t)P.n * P.nwin) / P.seg + 1);
  return P;
}

// Buckets per thread of the first reduction stage (msm_reduce1).  16 keeps the chunk records (two accumulators per
// chunk) and reduce2's work small where the reduction is throughput: a 2^20 proof's 352 k buckets.  A small bucket set
// (a shard's point sets, a small MSM) is a latency chain on a mostly empty GPU: with 4 the chain of reduce1 is 8
// additions instead of 32 and reduce2, run wide, pays 2 more scan steps (a G2 addition is ~20 us of wave time).
inline uint32_t msm_red_chunk(const MsmParams& P, const G16Env& env) {
  if (env.red_chunk) return (uint32_t)env.red_chunk;
  return P.nbuckets <= (1u << 17) ? 4u : 16u;
}

// ---- the sort phase -------------------------------------------------------------------------------------------------
struct MsmSortPlan {
  uint32_t lo_bits;   // low bucket bits sorted inside a partition
  uint32_t nparts;    // partitions = nbuckets >> lo_bits
  uint32_t ptiles;    // workgroups of a partition pass
  size_t nth;         // (partition, tile) histogram cells
  bool use_part;      // the partition sort; else the global-atomic histogram + scatter
  bool fused;         // bucket_place also does the split-bucket bookkeeping and the size histogram
  uint32_t nblk;      // grids: msm_count / msm_scatter,
  uint32_t ntiles;    //   the scan over the buckets,
  uint32_t nt2;       //   the scan over the histogram cells,
  uint32_t pblk;      //   perm_hist / perm_scatter
};
inline MsmSortPlan msm_sort_plan(const MsmParams& P, const G16Env& env) {
  MsmSortPlan L;
  // partition sort (see msm.cuh): low bits <= BS_LOG (as many as divide the bucket count: the class set of a
  // registered set is 43 * 2^(c-7) buckets), partitions = nwin << hi_bits
  L.lo_bits = P.c - 1 < (uint32_t)BS_LOG ? P.c - 1 : (uint32_t)BS_LOG;
  while (L.lo_bits && (P.nbuckets & ((1u << L.lo_bits) - 1))) --L.lo_bits;
  L.nparts = P.nbuckets >> L.lo_bits;
  L.ptiles = (P.n + PART_TILE - 1) / PART_TILE;
  L.use_part = L.nparts <= PART_MAX && env.msm_sort != 'a';
  L.nth = (size_t)L.nparts * L.ptiles;
  // lo_bits == BS_LOG: bucket_place also produces xoff / heavy / the size histogram (see msm.cuh); count[] and
  // offset[] are fully written by it, so the partition path clears only the two small counter blocks
  L.fused = L.use_part && L.lo_bits == (uint32_t)BS_LOG;
  L.nblk = (P.n + MSM_BLOCK - 1) / MSM_BLOCK;
  L.ntiles = (P.nbuckets + SCAN_TILE - 1) / SCAN_TILE;
  L.nt2 = (uint32_t)((L.nth + SCAN_TILE - 1) / SCAN_TILE);
  L.pblk = (P.nbuckets + PERM_BLOCK - 1) / PERM_BLOCK;
  return L;
}

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

// S: whatever holds the part pointers (g16_ctx::MsmSort on the host, a mirror struct in the CPU shim)
template <class S, class Carve>
void msm_sort_layout(S& s, const MsmParams& P, const MsmSortPlan& L, Carve& part) {
  const size_t nb = P.nbuckets;
  part(s.count, nb * 4);   // count + cursor are adjacent: one memset clears both
  part(s.cursor, nb * 4);
  part(s.offset, (nb + 1) * 4);
  part(s.xoff, nb * 4);
  part(s.heavy, nb * 4);
  part(s.info, 64);
  part(s.tiles, ((nb + SCAN_TILE - 1) / SCAN_TILE) * 8);
  part(s.entries, (size_t)P.n * P.nwin * 4);
  part(s.xseg, (size_t)P.max_extra * 8);
  part(s.perm, nb * 4);
  part(s.ghist, PERM_BINS * 4);
  part(s.blk_base, ((nb + PERM_BLOCK - 1) / PERM_BLOCK) * PERM_BINS * 4);
  part(s.tile_hist, L.use_part ? L.nth * 4 : 4);
  part(s.tmp, L.use_part ? (size_t)P.n * P.nwin * 8 : 8);
  part(s.tiles2, ((L.nth + SCAN_TILE - 1) / SCAN_TILE) * 8 + 8);
  part(s.slice_hist, L.use_part ? (size_t)L.nparts * BS_SPLIT * BS_LOW * 4 : 4);
}

// workspace of a job of msm_batch (the bucket sums come first: g16_msm_partial_ptr).  asz / psz29: bytes of a standard
// XYZZ accumulator (chunk sums and later: 128 / 256) and of a reduced-radix one (bucket sums: 144 / 288)
template <class J, class Carve>
void msm_job_layout(J& j, const MsmParams& P, size_t nchunks, size_t asz, size_t psz29, Carve& part) {
  part(j.partial, ((size_t)P.nbuckets + P.max_extra) * psz29);
  part(j.chunkR, nchunks * asz);
  part(j.chunkA, nchunks * asz);
  part(j.wsum, (size_t)(2 * 64 + 2) * asz);
}

// ---- the tail: split-bucket combine, reduce1, reduce2, fold -----------------------------------------------------------
enum class MsmR2 { QUAD128, QUAD64, WIDE, NARROW, WAVE };           // which msm_reduce2<C, Quad / Lane, slots>
enum class MsmFold { CLASSES_QUAD, CLASSES, MERGED, PLAIN };        // which msm_fold*
struct MsmTailPlan {
  uint32_t rc;          // buckets per chunk (msm_red_chunk)
  size_t nchunks;       // nbuckets / rc
  uint32_t nsets;       // reduction sets: workgroups of reduce2, inputs of the fold
  uint32_t log2ks;      // log2 of the buckets per set (merged / class bucket sets; 0: the sets are the windows)
  uint32_t cps;         // chunks per set
  MsmR2 r2;
  uint32_t r2_threads;  // workgroup size of r2
  uint32_t r2_lds;      // its dynamic LDS, in standard accumulators
  MsmFold fold;
  int heavy_forced;     // G16_HEAVY_GRID
  // Grid size of msm_heavy: the kernel loops grid-stride over the list of split buckets (all but empty for uniform or
  // circom-like scalars).  In the timeline of a proof this launch looks expensive (milliseconds, against 0.05 ms alone)
  // because its workgroups queue behind the accumulate waves of the other streams; shrinking the grid to 128 workgroups
  // was measured in round 2 (profiles/r02_ab_heavy_grid.txt): no change in proofs/s or latency -- the in-order reduce
  // behind it waits for the same slots -- and 30 % slower MSMs for scalars with thousands of split buckets
  // (tools/perf_skew.py "256 values": 3.92 -> 5.11 ms).
  uint32_t heavy_grid(uint32_t ny) const { return heavy_forced ? (uint32_t)heavy_forced : (ny > 1 ? 512u : 1024u); }
};
// narrow_tail: the caller overlaps this tail with other work (only read for the one-lane kernels, below)
inline MsmTailPlan msm_tail_plan(const MsmParams& P, bool is_g1, bool narrow_tail, const G16Env& env) {
  MsmTailPlan T;
  T.rc = msm_red_chunk(P, env);
  T.nchunks = P.nbuckets / T.rc;
  T.heavy_forced = env.heavy_grid;
  // reduction sets: the windows themselves, or <= 64 slices of the merged bucket set.  reduce2 is a latency chain
  // whose length grows with the chunks per thread, so the slices are as small as the 64 lanes of msm_fold_merged
  // allow: 512 chunks (2^13 buckets) per slice at c = 20 -> 64 workgroups, one chunk per thread (G1) / two (G2).
  // G16_RED_SLICE = log2(chunks per slice) overrides it (experiments).
  // A lean set (MsmParams::tstride >= 2) is reduced like a plain MSM of tstride windows: its bucket sets are the
  // residues r of the windows modulo the stride, and the fold applies 2^(c r) by Horner.
  const bool lean = P.tables && P.tstride >= 2;
  T.nsets = P.nwin;
  T.log2ks = 0;
  if (lean) {
    T.nsets = P.tstride;
  } else if (P.tables && P.mtab == 2) {   // class bucket set: 43 slices of 2^(c-7) buckets (msm_class_bucket)
    T.nsets = MSM_CLASS_SLICES;
    T.log2ks = P.c - 7;
  } else if (P.tables) {
    const uint32_t want = 1u << (env.red_slice_log2 ? env.red_slice_log2 : 9);
    uint32_t cps = T.nchunks < want ? (uint32_t)T.nchunks : want;
    while (T.nchunks / cps > 64) cps <<= 1;
    T.nsets = (uint32_t)(T.nchunks / cps);
    for (uint32_t ks = cps * T.rc; ks > 1; ks >>= 1) ++T.log2ks;
  }
  T.cps = (uint32_t)(T.nchunks / T.nsets);
  // reduce2 is a latency chain (serial chunk sums -> Hillis-Steele suffix scan -> tree).
  // Default: a cooperating quad per slot (Quad, msm.cuh: an addition in 4 multiplications of wave time instead of 14;
  // tools/ubench_quad.hip: 2.1-2.4 x per operation), 64 slots per slice (128 for G1 slices of >= 512 chunks; G2 at 512
  // threads would have to live in 256 registers).  Shards: 2.71-2.94 -> 2.61-2.82 ms per rank at G = 8; stand-alone 2^20
  // MSM 2.18 -> 2.00 ms (G1), 5.21 -> 4.87 (G2); 2^20 proofs: single-proof latency 10.79 -> 10.59 and 10.84 -> 10.54 ms in
  // two sessions, proofs/s 121.57 -> 120.91 and 119.23 -> 120.63, i.e. inside the noise (profiles/r04_ab_tail_quad.txt,
  // r04_ab_g2first_2p20.txt, r04_perf_reg_quad.txt).
  // G16_TAIL_QUAD=0 or any G16_R2_WIDTH selects one lane per slot (Lane, the form of rounds 1-3) and the wave-shuffle
  // fold.  There every scan step costs one group addition on EVERY wave of the workgroup: wide workgroups (512 / 256
  // threads: one chunk per thread) have the shortest chain; narrow ones (128 / 64 threads: four chunks per thread,
  // work-efficient serial sums, a 7- / 6-step scan) issue ~2.5x fewer wave-instructions for a ~20 % longer chain and
  // were the choice inside proofs (same-box A/B, profiles/r03_ab_knobs.txt: 111.6 -> 114.7 proofs/s, 11.67 -> 11.85
  // ms), wide for stand-alone MSMs and for 4-bucket chunks.  G16_R2_WIDTH = 0 / 1 / 2 forces wide / narrow / a single
  // wave per slice.
  const uint32_t wide = is_g1 ? 512u : 256u;
  const bool quad = env.r2_width < 0 && env.tail_quad != 0;
  if (quad) {
    T.r2 = is_g1 && T.cps >= 512 ? MsmR2::QUAD128 : MsmR2::QUAD64;
    T.r2_lds = T.r2 == MsmR2::QUAD128 ? 128u : 64u;
    T.r2_threads = 4 * T.r2_lds;
  } else {
    const int width = env.r2_width >= 0 ? env.r2_width : (narrow_tail && T.rc > 4 ? 1 : 0);
    T.r2 = width == 0 ? MsmR2::WIDE : width == 2 ? MsmR2::WAVE : MsmR2::NARROW;
    T.r2_threads = T.r2 == MsmR2::WIDE ? wide : T.r2 == MsmR2::WAVE ? 64u : wide / 4;
    T.r2_lds = T.r2_threads;
  }
  if (lean)
    T.fold = MsmFold::PLAIN;   // msm_fold over nsets = tstride sums, c doublings between them
  else if (P.tables && P.mtab == 2)
    T.fold = quad ? MsmFold::CLASSES_QUAD : MsmFold::CLASSES;
  else
    T.fold = P.tables ? MsmFold::MERGED : MsmFold::PLAIN;
  return T;
}

}  // namespace g16
