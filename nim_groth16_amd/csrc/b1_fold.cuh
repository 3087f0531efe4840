// pointsB1 folded into pointsA1 (b1_fold_form, key_plan.hpp): the one point operation of key creation that the fold
// needs, in a header of its own so that the CPU test shim runs the very code the device runs.
#pragma once
#include "ec.cuh"

namespace g16 {

// b - a for two affine points of the reference layout ((0,0) = infinity), exact and in the canonical affine form:
//   equal points (or both at infinity)  -> (0,0)
//   one side at infinity                -> the other side, negated if that side is a
//   b == -a                             -> 2 b, through dbl_affine (inside madd)
//   everything else                     -> an unequal addition and one inversion
template <class C>
FF_HD typename C::Aff point_difference(const typename C::Aff& b, const typename C::Aff& a) {
  using F = typename C::Field;
  if (F::eq(a.x, b.x) && F::eq(a.y, b.y)) return C::aff_inf();
  if (C::is_inf(a)) return b;
  if (C::is_inf(b)) return C::neg(a);
  typename C::Acc acc = C::from_affine(b);
  C::madd(acc, C::neg(a));
  return C::to_affine(acc);
}

}  // namespace g16
