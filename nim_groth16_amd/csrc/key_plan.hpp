// The layout of a resident proving key (pkey.hip), decided as data: which index ranges a shard holds, how many of its C1
// slots are this library's padding, what stands in for pointsB1, and where the entry lists of the B sets come from.
// Everything here is a pure function of its arguments -- the knobs come in as a G16Env -- and plain C++ without a heap:
// the CPU test shim builds it with g++ and holds every rule to a restatement (tests/test_key_plan_cpu.py,
// tests/test_b1_fold_cpu.py), as for ntt_plan.hpp, msm_plan.hpp and proof_plan.hpp.  pkey.hip only carries them out.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "g16_env.hpp"

namespace g16 {

// ---- which indices a shard holds --------------------------------------------------------------------------------------
// contiguous index ranges per rank, b = (N * (k + 1)) div ntasks (msm.nim:107-115): shard `index` of `count` holds
// [lo, hi) of N wires (A1 / B1 / B2 / C1) or of N domain indices (H1)
struct KeyRange {
  size_t lo, hi;
  size_t size() const { return hi - lo; }
};
inline KeyRange shard_range(size_t N, uint32_t index, uint32_t count) {
  return KeyRange{(N * index) / count, (N * (index + 1)) / count};
}
// pointsC1 covers wires npubs+1 .. nvars-1 (zkey_types.nim:40) and is stored wire-aligned, with infinity in the slots of
// the public wires 0 .. npubs.  Of the slots of a shard's wire range, this many are that padding and not points of the key:
// key creation fills them, g16_pkey_inf_counts leaves them out.
inline size_t c1_padding(KeyRange w, uint32_t npubs) {
  const size_t pub_end = w.hi < (size_t)npubs + 1 ? w.hi : (size_t)npubs + 1;
  return pub_end > w.lo ? pub_end - w.lo : 0;
}

// ---- points at infinity -----------------------------------------------------------------------------------------------
// a point set (or the B1 / B2 pair) with n_inf of its n points at (0,0) holds enough of them for entry lists of its
// own to pay (G16_INF_COMPACT, g16_pkey)
inline bool points_sparse(size_t n_inf, size_t n, const G16Env& env) {
  return n_inf && n_inf * 100 >= (size_t)env.inf_compact_pct * n;
}
// pointsB1 folded into pointsA1 (g16_pkey, pkey.hip).  A1 and B1 meet the same scalars, so with D_i = B1_i - A1_i
//   MSM(w, B1) = MSM(w, A1) + MSM(w, D),
// and D_i is the point at infinity for every wire whose columns of A and B coincide (squarings, boolean checks).  The
// form a key takes, from counts over its WHOLE wire range of n wires (every shard of a key reaches the same answer):
//   live_b1 = #{B1_i != inf},  live_delta = #{B1_i != A1_i}
//   EMPTY  no live difference: the B1 accumulation runs against no table at all and leaves infinity
//   DELTA  D in place of B1, where D holds few enough live points that dropping the others would pay against B1 as it
//          stands by the rule of points_sparse: live_delta * 100 <= live_b1 * (100 - G16_INF_COMPACT) -- and where D's
//          run costs no more than B1's did.  D has no arrangement of its own: its run reads the arrangement of all n
//          pairs (ProofPlan::sort_b1; or, with a handful of live points, none at all: b1_sparse_run below), where an
//          addition is skipped only if all 64 lanes of a wave meet infinity, so it
//          costs up to min(n, 64 * live_delta) wave-level additions.  B1 as it stands costs n of them, or live_b1 where
//          the key's B sets run on their compacted arrangement (points_sparse over the B1 points at infinity).  Against
//          n, D never loses; against a compacted B1 it must have most waves empty: 64 * live_delta <= live_b1.
//   PLAIN  everything else (and every key under G16_B1_FOLD=0): B1 as registered
// In the first two forms the record's B1 slot holds MSM(w, D) and the combine kernel adds the A1 slots to it.
enum B1Form : int { B1_PLAIN = 0, B1_EMPTY = 1, B1_DELTA = 2 };
inline B1Form b1_fold_form(size_t live_b1, size_t live_delta, size_t n, const G16Env& env) {
  if (!env.b1_fold) return B1_PLAIN;
  if (live_delta == 0) return B1_EMPTY;
  const long long keep = 100 - (long long)env.inf_compact_pct;   // (G16_INF_COMPACT=101, "never": negative)
  if ((long long)live_delta * 100 > (long long)live_b1 * keep) return B1_PLAIN;
  const bool b1_compacted = n >= live_b1 && points_sparse(n - live_b1, n, env);
  if (b1_compacted && live_delta * 64 > live_b1) return B1_PLAIN;
  return B1_DELTA;
}
// How a DELTA key's B1 job accumulates.  Through the arrangement of all n pairs the run still costs one table gather per
// entry of that arrangement, whatever it finds.  With at most B1_SPARSE_MAX live differences over the whole wire range the
// key also keeps the list of its live wires, and the job's bucket sums come from the sparse run (msm_sparse_accum,
// msm.cuh), which reads those wires' scalars and nothing else: 64 wires x 13 windows of hits are a few KB of LDS.  Decided
// once per key, from the same whole-range count as the form, so every shard of a key reaches the same answer.  (0: no
// live difference -- such a key is EMPTY and has nothing to run.)
constexpr size_t B1_SPARSE_MAX = 64;
inline bool b1_sparse_run(size_t live_delta) { return live_delta != 0 && live_delta <= B1_SPARSE_MAX; }

// ---- the entry lists of the B sets ---------------------------------------------------------------------------------------
// B1 and B2 share one arrangement of the witness, so what it may leave out are the wires dead in BOTH sets.  Where that
// count (g16_pkey::deadB) and the bitmap of the others (g16_pkey::liveB) come from, for a shard of nw wires whose
// registered B1 / B2 sets hold bitmaps (every set of at least one point does):
//   LIVE_B2     DELTA form: the registered B1 set holds the differences, not pointsB1.  In a key B1_i = (0,0) <=>
//               B2_i = (0,0), so the union of the two bitmaps is B2's own, and only B2 reads that arrangement: the count
//               is B2's, known before anything is built, and the bitmap a copy of B2's
//   LIVE_UNION  the other forms: the OR of the two bitmaps, which also counts the dead wires
//   LIVE_NONE   nothing to decide from: no count (0), no lists
enum LiveSource : int { LIVE_NONE = 0, LIVE_B2 = 1, LIVE_UNION = 2 };
inline LiveSource live_b_source(int b1_form, size_t nw, bool b1_bitmap, bool b2_bitmap) {
  if (!nw || !b2_bitmap) return LIVE_NONE;
  if (b1_form == B1_DELTA) return LIVE_B2;
  return b1_bitmap ? LIVE_UNION : LIVE_NONE;
}
// ... and whether the key keeps that bitmap -- the B sets get entry lists of their own -- once `dead` is known.  From
// LIVE_B2 this is asked before the copy is made; from LIVE_UNION after the union has been computed, which is then dropped
// again if the pair is dense (nullptr = the sets ride on the shared witness sort).
inline bool live_b_kept(LiveSource source, size_t dead, size_t nw, const G16Env& env) {
  return source != LIVE_NONE && points_sparse(dead, nw, env);
}

}  // namespace g16
