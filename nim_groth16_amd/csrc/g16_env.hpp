// The experiment knobs of the library as plain data: no HIP, so that the launch plans that take them as an argument
// (msm_plan.hpp, key_plan.hpp, proof_plan.hpp) also build with g++ for the CPU tests.
#pragma once

// Experiment knobs (G16_* environment variables), read ONCE per process -- at the first g16_ctx_create -- and never
// again on the per-proof path.  0 / '\0' = not set.
struct G16Env {
  int msm_window = 0;      // G16_MSM_WINDOW   5..22: window bits of the one-shot MSMs
  int table_window = 0;    // G16_TABLE_WINDOW 5..22: window bits of registered point sets
  int msm_seg = 0;         // G16_MSM_SEG      8..4096: accumulate segment length
  char msm_sort = 0;       // G16_MSM_SORT     'a': atomic histogram/scatter instead of the partition sort
  int g1_lanes[3] = {3, 2, 0};   // G16_G1_LANES  lanes of the A1 / B1 / C1 MSMs (three digits from {0,2,3}).  C1 goes first,
                                 // on the sort's own lane: the H accumulation continues C1's bucket sums, so a late C1
                                 // delays the last chain of the proof (single-proof latency 11.2 -> 10.8 ms, same
                                 // throughput: profiles/r04_ab_g1_lanes.txt; rounds 1-3: 0, 2, 3)
  char stream_prio[7] = "lhllln";   // G16_STREAM_PRIO  six characters from {h, n, l}
  int red_slice_log2 = 0;  // G16_RED_SLICE    log2 of the chunks per reduce2 slice of a merged bucket set (8..11)
  int inf_compact_pct = 10;   // G16_INF_COMPACT  point sets with at least this percentage of (0,0) points get their own
                              // entry lists without them (0: always, 101: never); key_plan.hpp
  int r2_width = -1;       // G16_R2_WIDTH  0: reduce2 with 512 / 256-thread workgroups, 1: 128 / 64, 2: 64 / 64; unset:
                           // narrow inside proofs, wide for stand-alone MSMs (msm_stage.cuh)
  int ntt_tile = 2048;            // G16_NTT_TILE = 1024 | 2048 | 4096: NTT workgroup geometry (ntt.cuh)
  // launch order of a proof (the defaults are the measured optimum: profiles/r05_ab_quotient_first*.txt):
  int quotient_first = 1;         // G16_QUOTIENT_FIRST=0: enqueue the witness MSMs before buildABC + quotient + sort(qs) (rounds 1-4)
  int lanes_after_quotient = 0;   // G16_LANES_AFTER_QUOTIENT=1 (with the above): the witness accumulations wait for them
  int g1_batch = 0;               // G16_G1_BATCH=1: ONE batched launch sequence (blockIdx.y = MSM) for A1, B1, C1 on one stream
                                  // instead of one stream and one sequence per G1 MSM (proof_plan.hpp; measured slower)
  int mtab = 2;                   // G16_MTAB=1: registered sets without the second multiplier table / class bucket set
  int chain_ch = 1;               // G16_CHAIN_CH=0: C1 and H1 as two MSMs instead of H1 continuing C1's bucket sums
  int tail_quad = 1;              // G16_TAIL_QUAD=0: reduce2 / fold with one lane per slot instead of a cooperating quad
                                  // (Lane / Quad, msm.cuh; msm_stage.cuh)
  int red_chunk = 0;              // G16_RED_CHUNK = 2 | 4 | 8 | 16: buckets per thread of msm_reduce1 (unset: msm_red_chunk)
  int cu_split = 0;               // G16_CU_SPLIT=k (1..24): main stream on k CUs per XCD, MSM lanes on the other 32 - k (g16hip.hip)
  int heavy_grid = 0;             // G16_HEAVY_GRID: workgroups of msm_heavy (unset: 1024 / 512; msm_stage.cuh)
  int cz_on_the_fly = 1;          // G16_CZ_FLY=0: buildABC writes Cz with a kernel of its own instead of the quotient's first
                                  // pass forming it while loading (ntt.cuh mul_src)
  int abc_dict = 1;               // G16_ABC_DICT=0: buildABC reads a 32-byte value per entry even when the key's coefficients
                                  // come from a small set (spmv.hip: value dictionary)
  int g2_first = -1;              // G16_G2_FIRST = 0 | 1 | 2: A1 and B1 (2: C1 too) accumulate after B2 (unset: 1 for small shards,
                                  // proof_plan.hpp)
  int b1_fold = 1;                // G16_B1_FOLD=0: every key keeps pointsB1 as it is (b1_fold_form, key_plan.hpp: always PLAIN)
};
