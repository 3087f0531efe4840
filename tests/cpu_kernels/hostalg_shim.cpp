// Test-only: the host algebra of a proof's last step (csrc/host_curve.hpp: host_add, host_mul, host_mul2 and the two
// combine halves, over the 4 x u64 host field of csrc/host_ff64.hpp) compiled with g++, so that it can be held to Python
// integers on a machine without a GPU.  Not part of the product library.
#include "../../nim_groth16_amd/csrc/host_curve.hpp"
#include <cstring>
using namespace g16;

template <class T> static T ld(const void* p) { T t; std::memcpy(&t, p, sizeof(T)); return t; }
template <class T> static void st(void* p, const T& t) { std::memcpy(p, &t, sizeof(T)); }

// op: 0 add 1 sub 2 neg 3 dbl 4 mul 5 sqr 6 mulsub(a,b,c,d) 7 inv 8..11 mul_small by 2, 3, 4, 8 12 is_zero 13 eq
// (the two predicates give one() or zero()).  n elements per operand array, one result each.
template <class F>
static void field_batch(int op, size_t n, const char* a, const char* b, const char* c, const char* d, char* out) {
  using T = typename F::T;
  const size_t sz = sizeof(T);
  for (size_t i = 0; i < n; ++i) {
    const T x = ld<T>(a + sz * i), y = ld<T>(b + sz * i), z = ld<T>(c + sz * i), w = ld<T>(d + sz * i);
    T r;
    switch (op) {
      case 0: r = F::add(x, y); break;
      case 1: r = F::sub(x, y); break;
      case 2: r = F::neg(x); break;
      case 3: r = F::dbl(x); break;
      case 4: r = F::mul(x, y); break;
      case 5: r = F::sqr(x); break;
      case 6: r = F::mulsub(x, y, z, w); break;
      case 7: r = F::inv(x); break;
      case 8: r = F::mul_small(x, 2); break;
      case 9: r = F::mul_small(x, 3); break;
      case 10: r = F::mul_small(x, 4); break;
      case 11: r = F::mul_small(x, 8); break;
      case 12: r = F::is_zero(x) ? F::one() : F::zero(); break;
      default: r = F::eq(x, y) ? F::one() : F::zero(); break;
    }
    st(out + sz * i, r);
  }
}

// mode 0: acc += q_i over n affine points with the mixed addition; mode 1: acc += q_i over n XYZZ records of `stride`
// bytes with the general addition, as prove_combine_kernel and sum_partials_kernel do; then the canonical affine form
template <class HC>
static void curve_sum(int mode, const char* p, size_t n, size_t stride, void* out) {
  typename HC::Acc acc = HC::acc_inf();
  for (size_t i = 0; i < n; ++i) {
    if (mode == 0) HC::madd(acc, ld<typename HC::Aff>(p + stride * i));
    else HC::add(acc, ld<typename HC::Acc>(p + stride * i));
  }
  st(out, HC::to_affine(acc));
}

extern "C" {
void shim_hfp_batch(int op, size_t n, const void* a, const void* b, const void* c, const void* d, void* out) {
  field_batch<HFp>(op, n, (const char*)a, (const char*)b, (const char*)c, (const char*)d, (char*)out);
}
void shim_hfp2_batch(int op, size_t n, const void* a, const void* b, const void* c, const void* d, void* out) {
  field_batch<HFp2>(op, n, (const char*)a, (const char*)b, (const char*)c, (const char*)d, (char*)out);
}
// the three host helpers exactly as prover.hip instantiates them: device affine types in and out; scalars in standard form
void shim_host_add(int group, const void* a, const void* b, void* out) {
  if (group == 1) st(out, host_add<HG1>(ld<g1_aff>(a), ld<g1_aff>(b)));
  else st(out, host_add<HG2>(ld<g2_aff>(a), ld<g2_aff>(b)));
}
void shim_host_mul(int group, const void* k_std, const void* p, void* out) {
  if (group == 1) st(out, host_mul<HG1>(ld<u256>(k_std), ld<g1_aff>(p)));
  else st(out, host_mul<HG2>(ld<u256>(k_std), ld<g2_aff>(p)));
}
void shim_host_mul2(int group, const void* k1_std, const void* p1, const void* k2_std, const void* p2, void* out) {
  if (group == 1) st(out, host_mul2<HG1>(ld<u256>(k1_std), ld<g1_aff>(p1), ld<u256>(k2_std), ld<g1_aff>(p2)));
  else st(out, host_mul2<HG2>(ld<u256>(k1_std), ld<g2_aff>(p1), ld<u256>(k2_std), ld<g2_aff>(p2)));
}
void shim_host_sum(int group, int mode, const void* p, size_t n, size_t stride, void* out) {
  if (group == 1) curve_sum<HG1>(mode, (const char*)p, n, stride, out);
  else curve_sum<HG2>(mode, (const char*)p, n, stride, out);
}
// the enqueue half's arithmetic: key constants and the mask (Montgomery) -> CombinePre (320 bytes)
void shim_combine_pre(const void* alpha1, const void* beta1, const void* delta1, const void* beta2, const void* delta2,
                      const void* r_mont, const void* s_mont, void* pre_out) {
  st(pre_out, host_combine_pre(ld<g1_aff>(alpha1), ld<g1_aff>(beta1), ld<g1_aff>(delta1), ld<g2_aff>(beta2),
                               ld<g2_aff>(delta2), ld<u256>(r_mont), ld<u256>(s_mont)));
}
// the finish half's: CombinePre and the five affine MSM sums A1 | B1 | B2 | H1 | C1 (384 bytes) -> pi_a | pi_b | pi_c
void shim_combine_finish(const void* pre, const void* res, void* proof_out) {
  g1_aff pi_a, pi_c;
  g2_aff pi_b;
  host_combine_finish(ld<CombinePre>(pre), ld<CombineRes>(res), pi_a, pi_b, pi_c);
  st(proof_out, pi_a);
  st((char*)proof_out + 64, pi_b);
  st((char*)proof_out + 192, pi_c);
}
uint32_t shim_sizes(int which) { return which == 0 ? sizeof(CombinePre) : sizeof(CombineRes); }
}
