// The order-r test of the key audit, [r]Q == infinity, as DATA: the multiplier is the constant r, so the whole
// double / add schedule is known when the library is compiled and is the same in every lane (audit.cuh walks it; no
// lane ever looks at a scalar bit).  Plain C++17, no HIP: the CPU suite builds it with g++ and evaluates it.
//
// The schedule is the non-adjacent form of r, most significant digit first.  The ladder starts at acc = Q (the leading
// digit, always +1); step k then means: double `dbls` times, then add digit * Q (digit = +1 or -1).  r is odd, so the
// last step ends in an addition: for a point of order r it is (r -+ 1) Q +- Q, the opposite-operands path of the
// complete mixed addition.
#pragma once
#include <cstdint>

namespace g16 {

struct SubgroupStep {
  uint8_t dbls;   // doublings before the addition (>= 2: the digits are non-adjacent)
  int8_t digit;   // +1 / -1
};

struct SubgroupPlan {
  static constexpr int MAX_STEPS = 128;   // a 255-digit NAF has at most 128 non-zero digits
  int nsteps = 0;
  int ndbl = 0;   // doublings in all
  SubgroupStep step[MAX_STEPS] = {};
};

// r = 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001, little-endian 64-bit limbs
constexpr uint64_t SUBGROUP_R[4] = {0x43e1f593f0000001ull, 0x2833e84879b97091ull, 0xb85045b68181585dull,
                                    0x30644e72e131a029ull};

constexpr SubgroupPlan make_subgroup_plan() {
  uint64_t k[4] = {SUBGROUP_R[0], SUBGROUP_R[1], SUBGROUP_R[2], SUBGROUP_R[3]};
  int8_t naf[257] = {};
  int len = 0;
  while (k[0] | k[1] | k[2] | k[3]) {
    int d = 0;
    if (k[0] & 1) {
      d = 2 - (int)(k[0] & 3);   // +1 if k = 1 mod 4, -1 if k = 3 mod 4: k - d is a multiple of 4
      if (d > 0) {
        k[0] -= 1;               // k odd: no borrow
      } else {
        for (int i = 0; i < 4; ++i)
          if (++k[i]) break;     // carry while a limb wraps to zero
      }
    }
    naf[len++] = (int8_t)d;
    for (int i = 0; i < 3; ++i) k[i] = (k[i] >> 1) | (k[i + 1] << 63);
    k[3] >>= 1;
  }
  SubgroupPlan p;
  int dbls = 0;
  for (int i = len - 2; i >= 0; --i) {   // naf[len - 1] == +1 is the starting value acc = Q
    ++dbls;
    ++p.ndbl;
    if (naf[i]) {
      p.step[p.nsteps].dbls = (uint8_t)dbls;
      p.step[p.nsteps].digit = naf[i];
      ++p.nsteps;
      dbls = 0;
    }
  }
  return p;
}

inline constexpr SubgroupPlan SUBGROUP_PLAN = make_subgroup_plan();

// the plan evaluates to r: start at 1, per step shift left by dbls and add the digit (checked again, digit by digit
// and independently of this header's own arithmetic, by tests/test_key_audit_model_cpu.py)
constexpr bool subgroup_plan_is_r(const SubgroupPlan& p) {
  uint64_t k[4] = {1, 0, 0, 0};
  for (int s = 0; s < p.nsteps; ++s) {
    for (int b = 0; b < p.step[s].dbls; ++b) {
      if (k[3] >> 63) return false;
      for (int i = 3; i > 0; --i) k[i] = (k[i] << 1) | (k[i - 1] >> 63);
      k[0] <<= 1;
    }
    if (k[0] & 1) return false;   // the digit lands on an even value: no carry, no borrow
    if (p.step[s].digit > 0) k[0] += 1;
    else {
      for (int i = 0; i < 4; ++i)
        if (k[i]--) break;        // borrow while a limb was zero
    }
  }
  return k[0] == SUBGROUP_R[0] && k[1] == SUBGROUP_R[1] && k[2] == SUBGROUP_R[2] && k[3] == SUBGROUP_R[3];
}
static_assert(SUBGROUP_PLAN.nsteps > 0 && SUBGROUP_PLAN.step[SUBGROUP_PLAN.nsteps - 1].dbls > 0, "empty plan");
static_assert(subgroup_plan_is_r(SUBGROUP_PLAN), "the digit schedule does not evaluate to r");

}  // namespace g16
