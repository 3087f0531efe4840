// The launch schedule of a proof (prover.hip), decided once and as data: which kernels, copies, event records and waits
// go to which stream in which order, for the whole proof (g16_prove_partials) and for the two halves of a sharded one
// (g16_prove_partials_begin / _end).  Everything here is a pure function of its arguments -- the knobs come in as a
// G16Env, the key as a ProofShape -- and plain C++ without a heap: the CPU test shim builds it with g++ and holds every
// plan to a restated rule and to the ordering a proof's correctness rests on (tests/test_proof_plan_cpu.py), as it does
// for ntt_plan.hpp and msm_plan.hpp.  prover.hip only walks the step list.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "g16_env.hpp"
#include "key_plan.hpp"   // B1Form, b1_fold_form, points_sparse: what a key is, which a ProofShape restates

namespace g16 {

// ---- small decisions of the host layer that depend on the knobs alone ----------------------------------------------
// G16_CU_SPLIT=k: the CU mask of the main stream (`front`: k CUs of every XCD) or of an MSM lane (the other 32 - k).
// CU-mask bit i is CU (i / 8) of XCD (i % 8): the mask is dealt round robin over the XCCs.
inline void stream_cu_mask(const G16Env& env, bool front, uint32_t mask[8]) {
  for (int w = 0; w < 8; ++w) mask[w] = 0;
  for (int bit = 0; bit < 256; ++bit)
    if ((bit / 8 < env.cu_split) == front) mask[bit / 32] |= 1u << (bit % 32);
}
// G16_STREAM_PRIO: priority of stream `index` (0..4 = lanes, 5 = main) within the device's range [hi, lo] (numerically
// hi <= lo)
inline int stream_priority(const G16Env& env, int index, int lo, int hi) {
  switch (env.stream_prio[index]) {
    case 'h': return hi;
    case 'l': return lo;
    default: return (lo + hi) / 2;
  }
}

// ---- the schedule ----------------------------------------------------------------------------------------------------
// streams: the five MSM lanes (0: witness sort, 1: B2, 2, 3, 4: spare) and the context's main stream
constexpr int8_t PS_MAIN = 5;
// events: the cross-stream edges of a proof (g16_ctx::ev), then the `done` event of each lane
enum ProofEvent : int8_t { EV_NONE = -1, EV_A, EV_B, EV_Q, EV_B2, EV_C, EV_G2, EV_COUNT, EV_DONE0 = EV_COUNT };
// the five MSMs.  Each owns the accumulate workspace of one lane in every mode -- A1: 0, B1: 2, C1: 3, B2: 1, H: 4 -- and
// its slot of the partials record; A1, B1, C1 are adjacent so that one batched launch sequence can take all three.
enum ProofRun : int8_t { RUN_A1, RUN_B1, RUN_C1, RUN_B2, RUN_H, RUN_COUNT };
// the bucket arrangements (g16_ctx::sort): the witness (all pairs), the H scalars, the witness over A1's live pairs,
// the witness over the live pairs of B1 / B2
enum ProofSort : int8_t { SORT_W = 0, SORT_H = 1, SORT_WA = 2, SORT_WB = 3 };

enum ProofOp : uint8_t {
  OP_UPLOAD,      // witness -> HBM, partials record cleared (an empty range stays XYZZ infinity)
  OP_WAIT,        // a: event
  OP_RECORD,      // a: event
  OP_SORT_W,      // a: sort slot, b: live bitmap (0: none, 1: A1's, 2: the B1 | B2 union), c: the run whose table config
  OP_SORT_H,
  OP_BUILD_ABC,   // a: need_cz
  OP_QUOTIENT,    // a: Cz formed on the fly
  OP_COSET,       // a: which of Az / Bz / Cz (_begin)
  OP_POINTWISE,   // (_end)
  OP_MSM,         // a: first run, b: n_accum, c: n_tail, d: after_heavy event or EV_NONE, e: H continues C1's bucket sums
  OP_COPY_OUT,
  OP_HOST_SYNC,
};
struct ProofStep {
  uint8_t op;
  int8_t stream;
  int8_t a, b, c, d, e;
};

enum ProofEntry : int { PROOF_WHOLE, PROOF_BEGIN, PROOF_END };
struct ProofShape {
  size_t nw, nh;      // wires / domain indices of this key's ranges
  uint32_t log2n;
  bool liveA, liveB;  // the key has entry lists of its own for A1 / for B1 and B2
  bool cfg_equal;     // C1 and H1 are registered over the same bucket set
  int b1_form = B1_PLAIN;   // what the key's B1 set holds (b1_fold_form)
};

// Small witness ranges (the shards of a proof spread over GPUs): the four accumulations together do not fill the GPU,
// every kernel is a latency chain and B2's -- G2 additions, ~4 x the wave time of G1's -- is the longest: its
// accumulation goes first, next to C1's only (the H accumulation continues C1's bucket sums: the second longest chain);
// A1 and B1 then run under B2's reduce / fold tail.
constexpr size_t G2_FIRST_MAX = size_t(1) << 18;

constexpr int PROOF_PLAN_CAP = 48;
struct ProofPlan {
  int count = 0, cap = PROOF_PLAN_CAP;
  bool overflow = false;
  bool narrow_tail = true;   // proofs overlap their MSM tails with other work (msm_tail_plan)
  int8_t sort_a = SORT_W, sort_b = SORT_W;   // the arrangement A1 reads, and the one B1 and B2 read (C1: SORT_W, H: SORT_H)
  // ... unless B1 is folded into A1 (b1_fold_form): the difference set is live where A1 OR B1 is, which the B1 | B2
  // bitmap does not cover, so its run reads the arrangement of all pairs
  int8_t sort_b1 = SORT_W;
  ProofStep steps[PROOF_PLAN_CAP];

  void push(ProofOp op, int stream, int a = 0, int b = 0, int c = 0, int d = 0, int e = 0) {
    if (count >= cap || count >= PROOF_PLAN_CAP) {
      overflow = true;
      return;
    }
    steps[count++] = ProofStep{(uint8_t)op, (int8_t)stream, (int8_t)a, (int8_t)b, (int8_t)c, (int8_t)d, (int8_t)e};
  }
  void record(int stream, int ev) { push(OP_RECORD, stream, ev); }
  // A wait that is already in force -- the same stream waited for the same event and the event has not been recorded
  // again since -- is a no-op and is not issued twice.
  void wait(int stream, int ev) {
    for (int i = count - 1; i >= 0; --i) {
      const ProofStep& s = steps[i];
      if ((s.op == OP_RECORD && s.a == ev) || (s.op == OP_MSM && s.d == ev)) break;
      if (s.op == OP_WAIT && s.stream == stream && s.a == ev) return;
    }
    push(OP_WAIT, stream, ev);
  }
  void msm(int stream, int first, int n_accum, int n_tail, int after_heavy = EV_NONE, bool continues_c1 = false) {
    push(OP_MSM, stream, first, n_accum, n_tail, after_heavy, continues_c1);
  }
};

// C1 and H1 enter the proof only as their sum (pi_c = ... + H + C, prover.nim:301-302), and both point sets are
// registered with the same window, i.e. over the same bucket set: the H accumulation then STARTS from C1's bucket sums
// instead of from infinity, and the pair needs one bucket reduction (reduce1 / reduce2 / fold) instead of two.  The
// C1 slot of the record stays at infinity.  G16_CHAIN_CH=0 restores two separate MSMs.
inline bool proof_chains_c_into_h(const G16Env& env, const ProofShape& s) {
  return env.chain_ch && s.nw && s.nh && s.cfg_equal;
}
// lanes that carry witness MSMs, and are joined at the end: 0 .. n - 1
inline int proof_witness_lanes(const G16Env& env) { return env.g1_batch ? 2 : 4; }

// The four MSMs that consume the witness (A1, B1, B2, C1: prover.nim:282, 288, 294, 302) on the lane streams.  The
// witness' signed-digit bucket arrangement is computed once (lane 0) and shared; the four accumulate / reduce pipelines
// run on four streams so that their latency-bound tails overlap the other pipelines' accumulation.  Nothing is waited
// for here.  Round 4 measured four other schedules against this one, same box, same session (profiles/r04_ab_*.txt):
//  * A1, B1, C1 as ONE batched launch sequence on one stream (every stage kernel takes blockIdx.y = MSM: three-wide
//    tails, 15 launches and 2 streams less): 110.2 vs 115.2 proofs/s.  Kept as G16_G1_BATCH=1.
//  * one accumulate stream per context with the tails on the lanes (a context then offers one accumulate kernel at a
//    time): 110.7 vs 117.4, and 33 / 10 proofs/s with 4 / 5 proofs in flight (the runtime's cross-stream waits stall).
//  * one accumulate stream for ALL in-flight proofs of the device: 8-12 proofs/s (stalls of 10-45 ms at the waits).
//  * an admission gate (the whole front of a proof -- upload, both sorts, buildABC, quotient -- first, then at most n
//    proofs past the gate, 4-6 in flight): 119.2-120.2 vs 119.5 -- the share of wall time without a resident
//    accumulate kernel falls from 12 % to 8 % (tools/overlap.py) and the throughput does not move.
// The step is bound by the instructions of ALL its kernels; what these schedules rearrange is latency.
// `after`: an event the accumulations wait for in addition to the sort -- the quotient's last kernel
// (G16_LANES_AFTER_QUOTIENT) -- or EV_NONE.
inline void proof_plan_witness(ProofPlan& p, const G16Env& env, const ProofShape& s, int after) {
  if (!s.nw) return;
  // phase 1: the bucket arrangements of the witness (lane 0)
  p.wait(0, EV_A);
  p.push(OP_SORT_W, 0, SORT_W, 0, RUN_A1);
  if (s.liveA) p.push(OP_SORT_W, 0, SORT_WA, 1, RUN_A1);   // A1 with many (0,0) points: its own arrangement, behind the shared one
  p.record(0, EV_B);
  // B1 / B2 with many (0,0) points: their own arrangement of the witness (live pairs only), built on B2's lane
  // while lane 0 arranges the full witness
  if (s.liveB) {
    p.wait(1, EV_A);
    p.push(OP_SORT_W, 1, SORT_WB, 2, RUN_B2);
    p.record(1, EV_B2);
  }
  // phase 2: accumulate + reduce A1, B1, B2, C1 against them
  const bool batch = env.g1_batch != 0;
  const bool chain = proof_chains_c_into_h(env, s);
  const int nlanes = proof_witness_lanes(env);
  // lanes of the three G1 MSMs; G16_G1_LANES reassigns them
  const int la = batch ? 0 : env.g1_lanes[0], lb = batch ? 0 : env.g1_lanes[1], lc = batch ? 0 : env.g1_lanes[2];
  for (int i = 1; i < nlanes; ++i) p.wait(i, i == 1 && s.liveB ? EV_B2 : EV_B);   // (lane 1 sorted for itself when B is sparse)
  if (s.liveB) p.wait(lb, EV_B2);
  // (A1's own arrangement lies on lane 0 ahead of EV_B: lanes 2 and 3 have waited for it above)
  if (after != EV_NONE)
    for (int i = 0; i < nlanes; ++i) p.wait(i, after);
  const bool g2_first = env.g2_first >= 0 ? env.g2_first != 0 : s.nw <= G2_FIRST_MAX;
  p.msm(1, RUN_B2, 1, 1, g2_first ? EV_G2 : EV_NONE);
  if (g2_first) {
    p.wait(la, EV_G2);
    p.wait(lb, EV_G2);
    if (!chain || env.g2_first == 2) p.wait(lc, EV_G2);
  }
  const int after_c = chain ? EV_C : EV_NONE;   // C1's bucket sums are final: H continues them, C1 has no tail of its own
  if (batch) {
    p.msm(0, RUN_A1, 3, chain ? 2 : 3, after_c);
  } else {
    p.msm(la, RUN_A1, 1, 1);
    p.msm(lb, RUN_B1, 1, 1);
    p.msm(lc, RUN_C1, 1, chain ? 0 : 1, after_c);
  }
  for (int i = 0; i < nlanes; ++i) p.record(i, EV_DONE0 + i);
}

// the H MSM over this key's domain range (prover.nim:301), then join the lanes and hand out the five partials
inline void proof_plan_h_and_collect(ProofPlan& p, const G16Env& env, const ProofShape& s, bool sorted, bool host_sync) {
  if (s.nh) {
    if (!sorted) p.push(OP_SORT_H, PS_MAIN);
    // G16_CU_SPLIT: the main stream owns a few CUs per XCD only; the H accumulation then runs on the spare lane (the
    // large partition), ordered behind the H sort and joined again below
    const int hs = env.cu_split ? 4 : PS_MAIN;
    if (hs != PS_MAIN) {
      p.record(PS_MAIN, EV_Q);
      p.wait(hs, EV_Q);
    }
    const bool chain = proof_chains_c_into_h(env, s);
    if (chain) p.wait(hs, EV_C);
    p.msm(hs, RUN_H, 1, 1, EV_NONE, chain);
    if (hs != PS_MAIN) {
      p.record(hs, EV_DONE0 + 4);
      p.wait(PS_MAIN, EV_DONE0 + 4);
    }
  }
  if (s.nw)
    for (int i = 0; i < proof_witness_lanes(env); ++i) p.wait(PS_MAIN, EV_DONE0 + i);
  p.push(OP_COPY_OUT, PS_MAIN);
  if (host_sync) p.push(OP_HOST_SYNC, PS_MAIN);
}

// task_mask: the coset pipelines of _begin (bit 0: A, bit 1: B, bit 2: C).  host_sync: the entry ends with a host wait
// for the main stream.  cap: for the tests.  -> false if the schedule does not fit the plan (nothing is written past it)
inline bool proof_plan_build(ProofPlan& p, const G16Env& env, ProofEntry entry, uint32_t task_mask, bool host_sync,
                             const ProofShape& s, int cap = PROOF_PLAN_CAP) {
  p = ProofPlan();
  p.cap = cap;
  p.sort_a = s.liveA ? SORT_WA : SORT_W;
  p.sort_b = s.liveB ? SORT_WB : SORT_W;
  p.sort_b1 = s.b1_form == B1_PLAIN ? p.sort_b : SORT_W;
  if (entry == PROOF_END) {
    p.push(OP_POINTWISE, PS_MAIN);
    proof_plan_h_and_collect(p, env, s, false, host_sync);
    return !p.overflow;
  }
  p.push(OP_UPLOAD, PS_MAIN);
  p.record(PS_MAIN, EV_A);   // witness resident
  if (entry == PROOF_BEGIN) {
    // this rank's coset pipelines go to the GPU first: every other rank waits for their slices
    if (task_mask) p.push(OP_BUILD_ABC, PS_MAIN, (task_mask & 4u) != 0);
    for (int v = 0; v < 3; ++v)
      if (task_mask & (1u << v)) p.push(OP_COSET, PS_MAIN, v);
    int after = EV_NONE;
    if (task_mask && env.quotient_first && env.lanes_after_quotient) p.record(PS_MAIN, after = EV_Q);
    proof_plan_witness(p, env, s, after);
    if (host_sync) p.push(OP_HOST_SYNC, PS_MAIN);   // the task outputs are complete; the lanes run on
    return !p.overflow;
  }
  // Launch order.  Rounds 1-4 enqueued the four witness MSMs first and buildABC + quotient + H behind them on the main
  // stream: with the thread-per-row buildABC of those rounds the other order lost (r02: 107.6-108.5 vs 107.9-110.4
  // proofs/s, 13.1 vs 12.0 ms single proof).  Since round 5 the head of the longest dependency chain -- buildABC (one
  // row-balanced launch) -> quotient (Cz formed on the fly) -> sort(qs) -> H MSM -- goes to the GPU BEFORE the ~60
  // launches of the witness lanes: two sessions, same box, identical proof bytes: single proof 10.61 -> 10.34 and
  // 10.67 -> 10.46 ms, proofs/s 121.5 -> 122.2 and 119.9 -> 120.3 (profiles/r05_ab_quotient_first*.txt).  Holding the
  // lanes back until the quotient is done (G16_LANES_AFTER_QUOTIENT=1) still loses (118.5, 11.4 ms).
  // G16_QUOTIENT_FIRST=0 restores the old order.  Replicated on every rank of a sharded proof unless the caller uses the
  // task-parallel pair g16_prove_partials_begin / _end.
  const int fly = s.log2n >= 1 && env.cz_on_the_fly ? 1 : 0;   // Cz formed by the quotient's first pass
  if (!env.quotient_first) proof_plan_witness(p, env, s, EV_NONE);
  p.push(OP_BUILD_ABC, PS_MAIN, fly == 0);
  p.push(OP_QUOTIENT, PS_MAIN, fly);
  if (env.quotient_first) {
    // ... and the bucket arrangement of the H scalars too: its dozen short kernels would otherwise queue, one after the
    // other, behind the GPU-filling accumulate waves of the four witness lanes (measured: 6 ms for a 0.5-ms sort)
    if (s.nh) p.push(OP_SORT_H, PS_MAIN);
    int after = EV_NONE;
    if (env.lanes_after_quotient) p.record(PS_MAIN, after = EV_Q);
    proof_plan_witness(p, env, s, after);
  }
  proof_plan_h_and_collect(p, env, s, env.quotient_first != 0, host_sync);
  return !p.overflow;
}

}  // namespace g16
