// Test-only: the rule that folds pointsB1 into pointsA1 (key_plan.hpp), what it changes in a proof's launch plan, and
// the device's point difference (b1_fold.cuh) compiled with g++.  Not part of the product library.
#include "../../nim_groth16_amd/csrc/b1_fold.cuh"
#include "../../nim_groth16_amd/csrc/proof_plan.hpp"
#include <cstring>
using namespace g16;

extern "C" {
// b1_fold_form of a key of n wires under G16_INF_COMPACT = pct and G16_B1_FOLD = fold
int shim_b1_fold_form(uint64_t live_b1, uint64_t live_delta, uint64_t n, int pct, int fold) {
  G16Env env;
  env.inf_compact_pct = pct;
  env.b1_fold = fold;
  return (int)b1_fold_form((size_t)live_b1, (size_t)live_delta, (size_t)n, env);
}
// the whole proof's plan of a key of the given shape and form: -> the arrangement its B1 run reads, or -1 if any step
// differs from the plan of the same key in the PLAIN form, or -2 if a plan does not fit
int shim_b1_plan(uint64_t nw, uint64_t nh, uint32_t log2n, int liveA, int liveB, int cfg_equal, int g1_batch, int form,
                 int* sort_b) {
  G16Env env;
  env.g1_batch = g1_batch;
  ProofShape s{(size_t)nw, (size_t)nh, log2n, liveA != 0, liveB != 0, cfg_equal != 0};
  ProofPlan plain, folded;
  if (!proof_plan_build(plain, env, PROOF_WHOLE, 0, true, s)) return -2;
  s.b1_form = form;
  if (!proof_plan_build(folded, env, PROOF_WHOLE, 0, true, s)) return -2;
  if (plain.count != folded.count || std::memcmp(plain.steps, folded.steps, sizeof(ProofStep) * plain.count) != 0) return -1;
  if (plain.sort_a != folded.sort_a || plain.sort_b != folded.sort_b || plain.narrow_tail != folded.narrow_tail) return -1;
  *sort_b = folded.sort_b;
  return folded.sort_b1;
}
// out = b - a over G1: 64-byte points of the reference layout (Montgomery)
void shim_g1_difference(const void* b, const void* a, void* out) {
  g1_aff pb, pa;
  std::memcpy(&pb, b, 64);
  std::memcpy(&pa, a, 64);
  const g1_aff d = point_difference<G1>(pb, pa);
  std::memcpy(out, &d, 64);
}
}
