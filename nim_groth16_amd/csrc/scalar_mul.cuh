// k * P by double-and-add, one lane per multiplication: the ladder of the verifier (pairing.hip) and of the circuit
// setup (circuit_setup.cuh).  The base point is affine (mixed additions) or an XYZZ accumulator (full additions: a
// butterfly of the group NTT multiplies a point that is already projective).  Every addition is the exact one of ec.cuh,
// so a base at infinity, k = 0 and a ladder that meets its own base again are all plain inputs.
#pragma once
#include "ec.cuh"

namespace g16 {

template <class C>
FF_HD void ladder_add(typename C::Acc& acc, const typename C::Aff& p) { C::madd(acc, p); }
template <class C>
FF_HD void ladder_add(typename C::Acc& acc, const typename C::Acc& p) { C::add(acc, p); }

// k * P over the 254 bits of a canonical scalar in standard form.  The leading zero limbs of k cost nothing and its
// leading zero bits one test each (doubling infinity returns at once), so a short scalar pays for its own length.
template <class C, class P>
FF_HD typename C::Acc scalar_mul(const P& p, u256 k) {
  typename C::Acc acc = C::acc_inf();
#pragma unroll 1
  for (int j = 7; j >= 0; --j) {
    uint32_t limb = k.v[7];
#pragma unroll
    for (int q = 7; q > 0; --q) k.v[q] = k.v[q - 1];   // rotate: static register indices
    k.v[0] = limb;
    if (limb == 0 && C::is_inf(acc)) continue;
#pragma unroll 1
    for (int b = 31; b >= 0; --b) {
      acc = C::dbl(acc);
      if ((limb >> b) & 1) ladder_add<C>(acc, p);
    }
  }
  return acc;
}

}  // namespace g16
