// The resident proving key: built by pkey.hip, read by the prover (prover.hip) and the prover pool (pool.hip).
#pragma once
#include "g16_internal.hpp"
#include "ec.cuh"

// Immutable after g16_pkey_create and tied to a DEVICE, not to the creating context: the in-flight proofs of one
// GPU (one g16_ctx each: private streams and workspaces) all prove against ONE resident key, and the key may be
// destroyed before or after any of those contexts (ProverPoints are per-circuit constants, zkey_types.nim:36-41).
struct g16_pkey {
  int device = 0;
  uint32_t nvars = 0, npubs = 0, log2n = 0, flavour = 1;
  // this key holds the index ranges [lo, hi) of each point set (shard_range, key_plan.hpp)
  uint32_t shard_index = 0, shard_count = 1;
  g16::KeyRange w{0, 0};   // A1 / B1 / B2 / C1 : range of wires (C1 is stored wire-aligned: c1_padding, key_plan.hpp)
  g16::KeyRange h{0, 0};   // H1                : range of domain indices
  g16_points *A1 = nullptr, *B1 = nullptr, *B2 = nullptr, *C1 = nullptr, *H1 = nullptr;
  // the A and B matrices (zkey section 4 / ZKey.coeffs, zkey_types.nim:48-59), row-binned for buildABC (spmv.hip)
  g16_spmat* abc = nullptr;
  size_t ncoeffs = 0;
  g16::g1_aff alpha1, beta1, delta1;
  g16::g2_aff beta2, delta2;
  // Points at infinity.  snarkjs keys hold (0,0) in pointsA1 / pointsB1 / pointsB2 for every wire absent from the
  // matrix (the loaders accept them, curves.nim:95-107; the MSMs sum over them, msm.nim:128-158).  In the shared
  // witness sort such an entry still occupies a loop trip of a wave whose other lanes run a full addition, so a set
  // with >= G16_INF_COMPACT % of them gets entry lists of its own that leave them out: liveA = A1's bitmap, liveB =
  // the union of B1's and B2's (one sort serves both; live_b_source, key_plan.hpp).  nullptr = dense: the set rides on
  // the shared sort.
  const uint32_t* liveA = nullptr;   // not owned: A1's own bitmap
  DevMem<uint32_t> liveB;            // owned, or empty
  size_t deadB = 0;                  // wires whose B1 AND B2 points are both (0,0)
  // pointsB1 folded into pointsA1 (b1_fold_form, key_plan.hpp).  B1_DELTA: `B1` holds the differences B1_i - A1_i
  // in place of pointsB1; B1_EMPTY: there is no live difference and the B1 accumulation runs against no table.  In both
  // the record's B1 slot holds MSM(w, difference) and the combine kernel adds the A1 slots to it.
  int b1_form = g16::B1_PLAIN;
  size_t b1_inf = 0;              // (0,0) points of pointsB1 itself in this key's wire range
  size_t live_b1 = 0, live_delta = 0;   // over the WHOLE wire range: what the form was decided from
  // B1_DELTA with few enough live differences (b1_sparse_run): the B1 job runs sparse.  One allocation: B1_VIEW_WORDS
  // zero words -- the job's view of an arrangement's counters, MsmJob::info: no extra segment, no split bucket -- then the
  // live wires of this shard's range, ascending and relative to its first wire (b1_nlive of them; a shard may hold none)
  static constexpr size_t B1_VIEW_WORDS = 16;
  DevMem<uint32_t> b1_sparse;   // empty: the run reads the arrangement of all pairs
  uint32_t b1_nlive = 0;
};
