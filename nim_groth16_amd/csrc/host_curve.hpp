// Host-only O(1) curve arithmetic of a proof's last step: the mask algebra of generateProofWithMask (reference
// groth16/prover.nim:279-302; done on the host there as well, curves.nim:136-214), regrouped into the part that needs
// the key and the mask alone and the part that needs the five MSM sums.  No HIP in here: prover.hip calls it, and
// tests/cpu_kernels/hostalg_shim.cpp compiles it with g++.
#pragma once
#include <string.h>

#include "ec.cuh"
#include "host_ff64.hpp"

namespace g16 {

// 64-bit-limb host field (host_ff64.hpp) under the same curve templates; 4-bit fixed windows.
using HG1 = Curve<HFp>;
using HG2 = Curve<HFp2>;
template <class HC, class DevAff>
static DevAff host_mul(const u256& k_std, const DevAff& p_dev) {
  static_assert(sizeof(DevAff) == sizeof(typename HC::Aff), "layout");
  typename HC::Aff p;
  memcpy(&p, &p_dev, sizeof p);
  typename HC::Acc tab[16];
  tab[0] = HC::acc_inf();
  tab[1] = HC::from_affine(p);
  for (int i = 2; i < 16; ++i) {
    tab[i] = tab[i - 1];
    HC::madd(tab[i], p);
  }
  typename HC::Acc acc = HC::acc_inf();
  for (int i = 7; i >= 0; --i)
    for (int nib = 7; nib >= 0; --nib) {
      if (!HC::is_inf(acc))
        for (int d = 0; d < 4; ++d) acc = HC::dbl(acc);
      uint32_t w = (k_std.v[i] >> (4 * nib)) & 15u;
      if (w) HC::add(acc, tab[w]);
    }
  typename HC::Aff r = HC::to_affine(acc);
  DevAff out;
  memcpy(&out, &r, sizeof out);
  return out;
}
template <class HC, class DevAff>
static DevAff host_add(const DevAff& a_dev, const DevAff& b_dev) {
  typename HC::Aff a, b;
  memcpy(&a, &a_dev, sizeof a);
  memcpy(&b, &b_dev, sizeof b);
  typename HC::Acc acc = HC::from_affine(a);
  HC::madd(acc, b);
  typename HC::Aff r = HC::to_affine(acc);
  DevAff out;
  memcpy(&out, &r, sizeof out);
  return out;
}
// k1 * p1 + k2 * p2 with ONE doubling chain (Shamir's trick, 2-bit joint windows: 16-entry table i*p1 + j*p2):
// 254 doublings + <= 127 additions instead of two separate 4-bit-window multiplications (512 + 156)
template <class HC, class DevAff>
static DevAff host_mul2(const u256& k1_std, const DevAff& p1_dev, const u256& k2_std, const DevAff& p2_dev) {
  typename HC::Aff p1, p2;
  memcpy(&p1, &p1_dev, sizeof p1);
  memcpy(&p2, &p2_dev, sizeof p2);
  typename HC::Acc tab[16];   // tab[4 i + j] = i*p1 + j*p2
  tab[0] = HC::acc_inf();
  for (int j = 1; j < 4; ++j) {
    tab[j] = tab[j - 1];
    HC::madd(tab[j], p2);
  }
  for (int i = 1; i < 4; ++i)
    for (int j = 0; j < 4; ++j) {
      tab[4 * i + j] = tab[4 * (i - 1) + j];
      HC::madd(tab[4 * i + j], p1);
    }
  typename HC::Acc acc = HC::acc_inf();
  for (int limb = 7; limb >= 0; --limb)
    for (int pos = 15; pos >= 0; --pos) {
      if (!HC::is_inf(acc)) acc = HC::dbl(HC::dbl(acc));
      const uint32_t w = 4 * ((k1_std.v[limb] >> (2 * pos)) & 3u) + ((k2_std.v[limb] >> (2 * pos)) & 3u);
      if (w) HC::add(acc, tab[w]);
    }
  typename HC::Aff r = HC::to_affine(acc);
  DevAff out;
  memcpy(&out, &r, sizeof out);
  return out;
}

// the five affine MSM sums as the combine kernel writes them
struct CombineRes {
  g1_aff a, b1;
  g2_aff b2;
  g1_aff h, c;
};
// the mask in standard form and the mask-only parts of the proof
struct CombinePre {
  u256 r_std, s_std;
  g1_aff a_pre;
  g2_aff b_pre;
  g1_aff c_pre;
};

// Everything that depends on the mask and the key alone (prover.nim:267-268, 279-302 regrouped):
//   pi_a = (alpha1 + r delta1) + A                      pi_b = (beta2 + s delta2) + B2
//   pi_c = s pi_a + r rho - rs delta1 + H + C           with rho = beta1 + s delta1 + B1
//        = (s alpha1 + r beta1 + rs delta1) + (s A + r B1) + H + C
// The same group elements as the reference's order of operations, hence the same canonical affine bytes.
// r, s: Montgomery form.
static inline CombinePre host_combine_pre(const g1_aff& alpha1, const g1_aff& beta1, const g1_aff& delta1,
                                          const g2_aff& beta2, const g2_aff& delta2, const u256& r, const u256& s) {
  CombinePre pre;
  pre.r_std = Fr::from_mont(r), pre.s_std = Fr::from_mont(s);
  const u256 rs_std = Fr::from_mont(Fr::mul(r, s));
  pre.a_pre = host_add<HG1>(alpha1, host_mul<HG1>(pre.r_std, delta1));
  pre.b_pre = host_add<HG2>(beta2, host_mul<HG2>(pre.s_std, delta2));
  pre.c_pre = host_add<HG1>(host_mul2<HG1>(pre.s_std, alpha1, pre.r_std, beta1), host_mul<HG1>(rs_std, delta1));
  return pre;
}

// What needs the MSM results -- three additions and ONE joint double-scalar multiplication.
static inline void host_combine_finish(const CombinePre& pre, const CombineRes& res, g1_aff& pi_a, g2_aff& pi_b,
                                       g1_aff& pi_c) {
  pi_a = host_add<HG1>(pre.a_pre, res.a);
  pi_b = host_add<HG2>(pre.b_pre, res.b2);
  pi_c = host_add<HG1>(pre.c_pre, host_mul2<HG1>(pre.s_std, res.a, pre.r_std, res.b1));
  pi_c = host_add<HG1>(pi_c, res.h);
  pi_c = host_add<HG1>(pi_c, res.c);
}

}  // namespace g16
