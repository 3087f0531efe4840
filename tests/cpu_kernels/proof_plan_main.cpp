// Builds every proof launch plan (proof_plan.hpp) of the grid of tests/test_proof_plan_cpu.py, each also at capacities
// below its length.  A stand-alone program: the test compiles it with -fsanitize=address,undefined, which makes it the
// bounds check of the plan's fixed-size step array.
//   proof_plan_main q,l,b,c,cu,cz,g2,la,lb,lc ...     one argument per knob set: quotient_first, lanes_after_quotient,
//                                                     g1_batch, chain_ch, cu_split, cz_on_the_fly, g2_first, g1_lanes
#include <cstdio>
#include <cstdlib>
#include <initializer_list>

#include "../../nim_groth16_amd/csrc/proof_plan.hpp"

using namespace g16;

static int fail(const char* what, const char* knobs) {
  std::printf("proof plan: %s (knobs %s)\n", what, knobs);
  return 1;
}

int main(int argc, char** argv) {
  const size_t nws[6] = {0, 1, 2046, size_t(1) << 18, (size_t(1) << 18) + 1, size_t(1) << 20};
  const size_t nhs[3] = {0, 1, size_t(1) << 11};
  const struct {
    ProofEntry entry;
    uint32_t task_mask;
  } entries[5] = {{PROOF_WHOLE, 0}, {PROOF_BEGIN, 0}, {PROOF_BEGIN, 5}, {PROOF_BEGIN, 7}, {PROOF_END, 0}};
  long built = 0;
  for (int a = 1; a < argc; ++a) {
    int v[10];
    if (std::sscanf(argv[a], "%d,%d,%d,%d,%d,%d,%d,%d,%d,%d", v, v + 1, v + 2, v + 3, v + 4, v + 5, v + 6, v + 7, v + 8,
                    v + 9) != 10)
      return fail("bad argument", argv[a]);
    G16Env env;
    env.quotient_first = v[0], env.lanes_after_quotient = v[1], env.g1_batch = v[2], env.chain_ch = v[3];
    env.cu_split = v[4], env.cz_on_the_fly = v[5], env.g2_first = v[6];
    for (int i = 0; i < 3; ++i) env.g1_lanes[i] = v[7 + i];
    for (size_t nw : nws)
      for (size_t nh : nhs)
        for (int live = 0; live < 4; ++live)
          for (int cfg_equal = 0; cfg_equal < 2; ++cfg_equal)
            for (uint32_t log2n : {0u, 11u})
              for (const auto& e : entries)
                for (int host_sync = 0; host_sync < 2; ++host_sync) {
                  const ProofShape s{nw, nh, log2n, (live & 1) != 0, (live & 2) != 0, cfg_equal != 0};
                  ProofPlan* full = new ProofPlan;   // on the heap: the sanitizer guards the bytes behind the array
                  if (!proof_plan_build(*full, env, e.entry, e.task_mask, host_sync != 0, s)) return fail("does not fit", argv[a]);
                  if (full->count < 2 || full->count > PROOF_PLAN_CAP) return fail("bad count", argv[a]);
                  for (int cap : {0, 1, full->count - 1, full->count, PROOF_PLAN_CAP + 1000}) {
                    ProofPlan* p = new ProofPlan;
                    const bool ok = proof_plan_build(*p, env, e.entry, e.task_mask, host_sync != 0, s, cap);
                    if (ok != (cap >= full->count)) return fail("capacity not reported", argv[a]);
                    if (p->count != (ok ? full->count : cap)) return fail("count past the capacity", argv[a]);
                    delete p;
                    ++built;
                  }
                  delete full;
                }
  }
  std::printf("proof plans ok %ld\n", built);
  return 0;
}
