// CPU build of the table-stride part of the MSM plan (msm_params.hpp, msm_plan.hpp) for tests/test_lean_tables_cpu.py:
// the slot function that the sort kernels index tables and bucket sets with, and the plan of a registered set at a
// stride next to the plan of the same set without one.
#include "../../nim_groth16_amd/csrc/msm_params.hpp"
#include "../../nim_groth16_amd/csrc/msm_plan.hpp"
#include <cstdint>

using namespace g16;

extern "C" {

// window w at table stride s -> out = {table, bucket set}
void shim_window_slot(uint32_t w, uint32_t s, uint32_t* out) { msm_window_slot(w, s, out[0], out[1]); }

// knobs: {msm_window, table_window, msm_seg, msm_sort, red_slice_log2, r2_width, mtab, tail_quad, red_chunk, heavy_grid}
static G16Env lean_env(const int* knobs) {
  G16Env env;
  env.msm_window = knobs[0];
  env.table_window = knobs[1];
  env.msm_seg = knobs[2];
  env.msm_sort = (char)knobs[3];
  env.red_slice_log2 = knobs[4];
  env.r2_width = knobs[5];
  env.mtab = knobs[6];
  env.tail_quad = knobs[7];
  env.red_chunk = knobs[8];
  env.heavy_grid = knobs[9];
  return env;
}

// what registration chooses for n points at `stride` (msm_table_choice): out = {c, mtab, stride, ntables, fits}
void shim_table_choice(uint64_t n, uint32_t stride, const int* knobs, uint32_t* out) {
  const MsmTableChoice t = msm_table_choice(n, stride, lean_env(knobs));
  out[0] = t.c, out[1] = t.mtab, out[2] = t.stride, out[3] = t.ntables, out[4] = t.fits ? 1u : 0u;
}

// The plans of an MSM of n pairs.  mode 0: a plain point array.  mode 1: a registered set as the stride-less callers
// describe it, table_cfg = c | mtab << 8.  mode 2: a registered set at `stride`, table_cfg = c | mtab << 8 | stride << 16:
// stride 0 or 1 beside the c and mtab of mode 1 (a stride of 1 is written out, not dropped), a larger one with the c, mtab
// and clamped stride of msm_table_choice.  out:
//   [0..9]   MsmParams  n c nwin nbuckets seg scalars_mont tables max_extra mtab tstride
//   [10..19] sort plan  lo_bits nparts ptiles nth use_part fused nblk ntiles nt2 pblk
//   [20..30] tail plan  rc nchunks nsets log2ks cps r2 r2_threads r2_lds fold heavy_grid(1) heavy_grid(3)
//   [31]     bytes of the sort workspace      [32] bytes of a job workspace (G1: 128- / 144-byte accumulators)
struct LeanSortParts {
  char *count, *cursor, *offset, *xoff, *heavy, *info, *tiles, *entries, *xseg, *perm, *ghist, *blk_base, *tile_hist, *tmp,
      *tiles2, *slice_hist;
};
struct LeanJobParts {
  char *partial, *chunkR, *chunkA, *wsum;
};
void shim_lean_plan(uint64_t n, uint32_t flags, int mode, uint32_t stride, int is_g1, int narrow_tail, const int* knobs,
                    uint64_t* out) {
  const G16Env env = lean_env(knobs);
  uint32_t cfg = 0;
  if (mode == 1) {
    const uint32_t c = msm_pick_table_window(n, env);
    cfg = c | (msm_pick_mtab(c, env) << 8);
  } else if (mode == 2 && stride < 2) {
    const uint32_t c = msm_pick_table_window(n, env);
    cfg = c | (msm_pick_mtab(c, env) << 8) | (stride << 16);
  } else if (mode == 2) {
    const MsmTableChoice t = msm_table_choice(n, stride, env);
    cfg = t.c | (t.mtab << 8) | (t.stride << 16);
  }
  const MsmParams P = msm_params(n, flags, cfg, env);
  const uint32_t p[10] = {P.n, P.c, P.nwin, P.nbuckets, P.seg, P.scalars_mont, P.tables, P.max_extra, P.mtab, P.tstride};
  for (int i = 0; i < 10; ++i) out[i] = p[i];
  const MsmSortPlan L = msm_sort_plan(P, env);
  const uint64_t l[10] = {L.lo_bits, L.nparts, L.ptiles, L.nth, L.use_part, L.fused, L.nblk, L.ntiles, L.nt2, L.pblk};
  for (int i = 0; i < 10; ++i) out[10 + i] = l[i];
  const MsmTailPlan T = msm_tail_plan(P, is_g1 != 0, narrow_tail != 0, env);
  const uint64_t t[11] = {T.rc, T.nchunks, T.nsets, T.log2ks, T.cps, (uint64_t)T.r2, T.r2_threads, T.r2_lds, (uint64_t)T.fold,
                          T.heavy_grid(1), T.heavy_grid(3)};
  for (int i = 0; i < 11; ++i) out[20 + i] = t[i];
  LeanSortParts S;
  Carver sort_size{nullptr};
  msm_sort_layout(S, P, L, sort_size);
  out[31] = sort_size.bytes;
  LeanJobParts J;
  Carver job_size{nullptr};
  msm_job_layout(J, P, T.nchunks, 128, 144, job_size);
  out[32] = job_size.bytes;
}

}  // extern "C"
