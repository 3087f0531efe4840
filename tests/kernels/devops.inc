// Test-only: the field / curve primitives of ff.cuh, ff29.cuh, ec.cuh, ec29.cuh, the tower and loops of pairing.cuh
// (and, under hipcc, msm_digits of msm.cuh) as numbered ops over flat 32-bit word buffers.  One call of Op<ID>::run
// handles ONE operand tuple of Op<ID>::in_words words and writes Op<ID>::out_words words.  FF_HD code only: included by
// the g++ shim (tests/cpu_kernels/devops_shim.cpp: the portable branches of the headers) and by tests/kernels/devops.hip
// (one kernel per op, one lane per tuple: the branches the GPU runs).  tests/device_ops.py builds the operands and the
// expected words from plain integers.  Every op is straight-line or has a fixed trip count, except the ones that reach
// Field::inv (field "inv", fp2 "inv", the to_affine at the end of the curve ops, the pairing ops that invert):
// canonical operands only.
//
// The including file has the headers included and `using namespace g16` is NOT assumed: everything is qualified.
namespace devops {

template <class T>
FF_HD T ldw(const uint32_t* p) {
  T t;
  __builtin_memcpy(&t, p, sizeof(T));
  return t;
}
template <class T>
FF_HD void stw(uint32_t* p, const T& t) {
  __builtin_memcpy(p, &t, sizeof(T));
}

template <int OP>
struct Op;
// carried: whether this build runs the op.  An op that is not carried keeps its number, name and sizes, its run() is
// never instantiated into a kernel, and running it is an error (see DEVOPS_PAIRING below).
#define DEVOP_IF(CARRIED, ID, NAME, INW, OUTW)                         \
  template <>                                                          \
  struct Op<ID> {                                                      \
    static constexpr const char* name() { return NAME; }               \
    static constexpr uint32_t in_words = (INW), out_words = (OUTW);    \
    static constexpr bool carried = (CARRIED);                         \
    static FF_HD void run(const uint32_t* in, uint32_t* out)
#define DEVOP(ID, NAME, INW, OUTW) DEVOP_IF(true, ID, NAME, INW, OUTW)
#define DEVOP_END };

// ---- Field<Fp> / Field<Fr>, 8 x 32 -----------------------------------------------------------------------------
// (a, b) canonical -> add sub mul sqr(a) neg(a) dbl(a) div2(a) from_mont(a) to_mont(a) mul_small(a, 2|3|4|8)
template <class F>
FF_HD void field_all(const uint32_t* in, uint32_t* out) {
  const g16::u256 a = ldw<g16::u256>(in), b = ldw<g16::u256>(in + 8);
  stw(out + 0, F::add(a, b));
  stw(out + 8, F::sub(a, b));
  stw(out + 16, F::mul(a, b));
  stw(out + 24, F::sqr(a));
  stw(out + 32, F::neg(a));
  stw(out + 40, F::dbl(a));
  stw(out + 48, F::div2(a));
  stw(out + 56, F::from_mont(a));
  stw(out + 64, F::to_mont(a));
  stw(out + 72, F::mul_small(a, 2));
  stw(out + 80, F::mul_small(a, 3));
  stw(out + 88, F::mul_small(a, 4));
  stw(out + 96, F::mul_small(a, 8));
}
// (a, b, c, d), each <= p -> mul2 mulsub neg_raw(a)
template <class F>
FF_HD void field_dot2(const uint32_t* in, uint32_t* out) {
  const g16::u256 a = ldw<g16::u256>(in), b = ldw<g16::u256>(in + 8), c = ldw<g16::u256>(in + 16), d = ldw<g16::u256>(in + 24);
  stw(out + 0, F::mul2(a, b, c, d));
  stw(out + 8, F::mulsub(a, b, c, d));
  stw(out + 16, F::neg_raw(a));
}
template <class F>
FF_HD void field_dot4(const uint32_t* in, uint32_t* out) {
  g16::u256 x[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) x[i] = ldw<g16::u256>(in + 8 * i);
  stw(out, F::mul4(x[0], x[1], x[2], x[3], x[4], x[5], x[6], x[7]));
}
// any two 256-bit integers -> geq(a, b) | is_canonical(a) << 1
template <class F>
FF_HD void field_cmp(const uint32_t* in, uint32_t* out) {
  const g16::u256 a = ldw<g16::u256>(in), b = ldw<g16::u256>(in + 8);
  out[0] = (F::geq(a, b) ? 1u : 0u) | (F::is_canonical(a) ? 2u : 0u);
}
template <class F>
FF_HD void field_inv(const uint32_t* in, uint32_t* out) { stw(out, F::inv(ldw<g16::u256>(in))); }
template <class F>
FF_HD void field_inv_fermat(const uint32_t* in, uint32_t* out) { stw(out, F::inv_fermat(ldw<g16::u256>(in))); }

DEVOP(0, "fp_all", 16, 104) { field_all<g16::Fp>(in, out); } DEVOP_END
DEVOP(1, "fr_all", 16, 104) { field_all<g16::Fr>(in, out); } DEVOP_END
DEVOP(2, "fp_dot2", 32, 24) { field_dot2<g16::Fp>(in, out); } DEVOP_END
DEVOP(3, "fr_dot2", 32, 24) { field_dot2<g16::Fr>(in, out); } DEVOP_END
DEVOP(4, "fp_dot4", 64, 8) { field_dot4<g16::Fp>(in, out); } DEVOP_END
DEVOP(5, "fr_dot4", 64, 8) { field_dot4<g16::Fr>(in, out); } DEVOP_END
DEVOP(6, "fp_cmp", 16, 1) { field_cmp<g16::Fp>(in, out); } DEVOP_END
DEVOP(7, "fr_cmp", 16, 1) { field_cmp<g16::Fr>(in, out); } DEVOP_END
DEVOP(8, "fp_inv", 8, 8) { field_inv<g16::Fp>(in, out); } DEVOP_END
DEVOP(9, "fr_inv", 8, 8) { field_inv<g16::Fr>(in, out); } DEVOP_END
DEVOP(10, "fp_inv_fermat", 8, 8) { field_inv_fermat<g16::Fp>(in, out); } DEVOP_END
DEVOP(11, "fr_inv_fermat", 8, 8) { field_inv_fermat<g16::Fr>(in, out); } DEVOP_END

// ---- Fp2 ---------------------------------------------------------------------------------------------------------
// (a, b) -> add sub mul sqr(a) mul_small(a, 2|3|4|8)
DEVOP(12, "fp2_all", 32, 128) {
  const g16::fp2_t a = ldw<g16::fp2_t>(in), b = ldw<g16::fp2_t>(in + 16);
  stw(out + 0, g16::Fp2::add(a, b));
  stw(out + 16, g16::Fp2::sub(a, b));
  stw(out + 32, g16::Fp2::mul(a, b));
  stw(out + 48, g16::Fp2::sqr(a));
  stw(out + 64, g16::Fp2::mul_small(a, 2));
  stw(out + 80, g16::Fp2::mul_small(a, 3));
  stw(out + 96, g16::Fp2::mul_small(a, 4));
  stw(out + 112, g16::Fp2::mul_small(a, 8));
} DEVOP_END
DEVOP(13, "fp2_mulsub", 64, 16) {
  stw(out, g16::Fp2::mulsub(ldw<g16::fp2_t>(in), ldw<g16::fp2_t>(in + 16), ldw<g16::fp2_t>(in + 32), ldw<g16::fp2_t>(in + 48)));
} DEVOP_END
DEVOP(14, "fp2_inv", 16, 16) { stw(out, g16::Fp2::inv(ldw<g16::fp2_t>(in))); } DEVOP_END

// ---- Field29 (9 x 29, raw limbs in and out) ----------------------------------------------------------------------
using F29 = g16::Fp29;
FF_HD g16::fe29 ld29(const uint32_t* in, int i) { return ldw<g16::fe29>(in + 9 * i); }

DEVOP(15, "f29_relimb_in", 8, 9) { stw(out, F29::relimb(ldw<g16::u256>(in))); } DEVOP_END      // any 256-bit integer
DEVOP(16, "f29_relimb_out", 9, 8) { stw(out, F29::relimb(ld29(in, 0))); } DEVOP_END            // canonical
DEVOP(17, "f29_from_std", 8, 9) { stw(out, F29::from_std(ldw<g16::u256>(in))); } DEVOP_END
DEVOP(18, "f29_to_std", 9, 8) { stw(out, F29::to_std(ld29(in, 0))); } DEVOP_END
DEVOP(19, "f29_mul", 18, 9) { stw(out, F29::mul(ld29(in, 0), ld29(in, 1))); } DEVOP_END
DEVOP(20, "f29_sqr", 9, 9) { stw(out, F29::sqr(ld29(in, 0))); } DEVOP_END
DEVOP(21, "f29_dot2", 36, 9) { stw(out, F29::dot2(ld29(in, 0), ld29(in, 1), ld29(in, 2), ld29(in, 3))); } DEVOP_END
DEVOP(22, "f29_dot4", 72, 9) {
  stw(out, F29::dot4(ld29(in, 0), ld29(in, 1), ld29(in, 2), ld29(in, 3), ld29(in, 4), ld29(in, 5), ld29(in, 6), ld29(in, 7)));
} DEVOP_END
// dot_pair<NP> as ec29.cuh instantiates it (NP = 1, 2, 4): operands a0 b0 .. a(NP-1) b(NP-1), c0 d0 .. ; the unused
// slots are filled with a0, as f2mul / f2sqr fill them with a live value
template <int NP>
FF_HD void f29_pair(const uint32_t* in, uint32_t* out) {
  g16::fe29 x[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) x[i] = ld29(in, i < 2 * NP ? i : (i >= 8 && i < 8 + 2 * NP) ? 2 * NP + (i - 8) : 0);
  g16::fe29 r0, r1;
  F29::dot_pair<NP>(r0, r1, x[0], x[1], x[2], x[3], x[4], x[5], x[6], x[7], x[8], x[9], x[10], x[11], x[12], x[13], x[14], x[15]);
  stw(out, r0);
  stw(out + 9, r1);
}
DEVOP(23, "f29_pair1", 36, 18) { f29_pair<1>(in, out); } DEVOP_END
DEVOP(24, "f29_pair2", 72, 18) { f29_pair<2>(in, out); } DEVOP_END
DEVOP(25, "f29_pair4", 144, 18) { f29_pair<4>(in, out); } DEVOP_END
// the carry-free linear ops, with the (MULT, LIFT) pairs ec29.cuh instantiates.  in: sel, a, b, c
//   0 add(a,b)  1 norm(a)  2..5 subk<16|4|32|8, 1>(a,b)  6 subk2<8,3>(a,b,c)  7..11 negk<2|4|8|16|32, 1>(b)
DEVOP(26, "f29_lin", 28, 9) {
  const g16::fe29 a = ld29(in + 1, 0), b = ld29(in + 1, 1), c = ld29(in + 1, 2);
  g16::fe29 r = F29::zero();
  switch (in[0]) {
    case 0: r = F29::add(a, b); break;
    case 1: r = F29::norm(a); break;
    case 2: r = F29::subk<16, 1>(a, b); break;
    case 3: r = F29::subk<4, 1>(a, b); break;
    case 4: r = F29::subk<32, 1>(a, b); break;
    case 5: r = F29::subk<8, 1>(a, b); break;
    case 6: r = F29::subk2<8, 3>(a, b, c); break;
    case 7: r = F29::negk<2, 1>(b); break;
    case 8: r = F29::negk<4, 1>(b); break;
    case 9: r = F29::negk<8, 1>(b); break;
    case 10: r = F29::negk<16, 1>(b); break;
    case 11: r = F29::negk<32, 1>(b); break;
    default: break;
  }
  stw(out, r);
} DEVOP_END
// in: MAXMULT (1 | 4 | 16), a normalized < 2 MAXMULT p.  out: canon<MAXMULT>(a), maybe_zero | is_zero_exact<MAXMULT> << 1
DEVOP(27, "f29_canon", 10, 10) {
  const g16::fe29 a = ld29(in + 1, 0);
  g16::fe29 r = F29::zero();
  uint32_t z = 0;
  switch (in[0]) {
    case 1: r = F29::canon<1>(a); z = F29::is_zero_exact<1>(a); break;
    case 4: r = F29::canon<4>(a); z = F29::is_zero_exact<4>(a); break;
    case 16: r = F29::canon<16>(a); z = F29::is_zero_exact<16>(a); break;
    default: break;
  }
  stw(out, r);
  out[9] = (F29::maybe_zero(a) ? 1u : 0u) | (z ? 2u : 0u);
} DEVOP_END

// ---- G1 / G2 of ec.cuh: sequences of up to 8 affine points -------------------------------------------------------
// in: count, mode, 2 pad words, 8 points.  out: the canonical affine result.
//   0 madd chain   1 add(from_affine) chain   2 mul_small(from_affine(p0), count)   3 count doublings of from_affine(p0)
//   4 dbl_affine(p0) (p0 finite)   5 neg(Acc) of the madd chain over neg(Aff): the same sum
template <class C>
FF_HD void ec_seq(const uint32_t* in, uint32_t* out) {
  constexpr int PW = sizeof(typename C::Aff) / 4;
  const uint32_t n = in[0], mode = in[1];
  const uint32_t* pts = in + 4;
  typename C::Acc acc = C::acc_inf();
  if (mode == 2) {
    acc = C::mul_small(C::from_affine(ldw<typename C::Aff>(pts)), n);
  } else if (mode == 3) {
    acc = C::from_affine(ldw<typename C::Aff>(pts));
    for (uint32_t i = 0; i < n && i < 8; ++i) acc = C::dbl(acc);
  } else if (mode == 4) {
    acc = C::dbl_affine(ldw<typename C::Aff>(pts));
  } else {
    for (uint32_t i = 0; i < n && i < 8; ++i) {
      const typename C::Aff q = ldw<typename C::Aff>(pts + PW * i);
      if (mode == 0) C::madd(acc, q);
      else if (mode == 1) C::add(acc, C::from_affine(q));
      else C::madd(acc, C::neg(q));
    }
    if (mode == 5) acc = C::neg(acc);
  }
  stw(out, C::to_affine(acc));
}
DEVOP(28, "g1_seq", 4 + 8 * 16, 16) { ec_seq<g16::G1>(in, out); } DEVOP_END
DEVOP(29, "g2_seq", 4 + 8 * 32, 32) { ec_seq<g16::G2>(in, out); } DEVOP_END

// ---- Ec29<G1> / Ec29<G2>: sequences of up to LEN affine points (8 x 32 layout in, canonical affine out) -------------
// in: count, mode, 2 pad words, LEN points.
//   0 acc += q through the packed table entry   1 acc += -(-q) through the sign flag
//   2 pairwise tree of XYZZ += XYZZ over one-point accumulators (both operands lazy; a stack holds one partial per level)
//   3 as 0, with acc = acc_from_std(to_std(acc)) after every addition   4 as 0, the entry repacked: pack(unpack(t))
template <class C, int LEN>
FF_HD void ec29_seq(const uint32_t* in, uint32_t* out) {
  using E = g16::Ec29<C>;
  constexpr int PW = sizeof(typename C::Aff) / 4;
  const uint32_t n = in[0] < (uint32_t)LEN ? in[0] : (uint32_t)LEN, mode = in[1];
  const uint32_t* pts = in + 4;
  typename E::Acc acc = E::acc_inf();
  if (mode == 2) {
    typename E::Acc st[10];   // LEN <= 2^9: at most one partial per level
    uint32_t depth = 0;
    for (uint32_t i = 0; i < n; ++i) {
      typename E::Acc a = E::acc_inf();
      const typename E::Tab t = E::tab_from_std(ldw<typename C::Aff>(pts + PW * i));
      E::madd(a, &t, 0u);
      for (uint32_t m = i; m & 1u; m >>= 1) {   // merge while this level already holds a partial
        typename E::Acc l = st[--depth];
        E::add(l, a);
        a = l;
      }
      st[depth++] = a;
    }
    while (depth > 0) {
      typename E::Acc l = st[--depth];
      E::add(l, acc);
      acc = l;
    }
  } else {
    for (uint32_t i = 0; i < n; ++i) {
      typename C::Aff q = ldw<typename C::Aff>(pts + PW * i);
      if (mode == 1) q = C::neg(q);
      typename E::Tab t = E::tab_from_std(q);
      if (mode == 4) t = E::pack(E::unpack(t));
      E::madd(acc, &t, mode == 1 ? 1u : 0u);
      if (mode == 3) acc = E::acc_from_std(E::to_std(acc));
    }
  }
  stw(out, C::to_affine(E::to_std(acc)));
}
DEVOP(30, "g1_seq29", 4 + 8 * 16, 16) { ec29_seq<g16::G1, 8>(in, out); } DEVOP_END
DEVOP(31, "g2_seq29", 4 + 8 * 32, 32) { ec29_seq<g16::G2, 8>(in, out); } DEVOP_END
DEVOP(32, "g1_chain29", 4 + 400 * 16, 16) { ec29_seq<g16::G1, 400>(in, out); } DEVOP_END
DEVOP(33, "g2_chain29", 4 + 400 * 32, 32) { ec29_seq<g16::G2, 400>(in, out); } DEVOP_END
// one affine point -> tab_from_std, pack(unpack(.)) of it: the packed table entries as they lie in memory
DEVOP(34, "g1_tab29", 16, 32) {
  using E = g16::Ec29<g16::G1>;
  const E::Tab t = E::tab_from_std(ldw<g16::g1_aff>(in));
  stw(out, t);
  stw(out + 16, E::pack(E::unpack(t)));
} DEVOP_END
DEVOP(35, "g2_tab29", 32, 64) {
  using E = g16::Ec29<g16::G2>;
  const E::Tab t = E::tab_from_std(ldw<g16::g2_aff>(in));
  stw(out, t);
  stw(out + 32, E::pack(E::unpack(t)));
} DEVOP_END

// ---- Pairing of pairing.cuh: the Fp12 tower, the Miller loop, the final exponentiation ------------------------------
// An Fp12 element is 96 words: g[0..5], six Fp2 values over w^k in Montgomery form (what g16_pairing returns); an Fp6
// element is 48 words, c[0..2] over v = w^2.  None of the arithmetic configuration macros reaches pairing.cuh except
// G16_FP2_CALLS, so only the builds whose configuration ships pairing.o carry these ops: the including file may define
// DEVOPS_PAIRING as 0 to leave them out (number, name and sizes stay, so the table is the same in every build).
// f12_inv, f6_inv, pair_miller and pair_final_exp reach Fp2::inv: canonical operands, and no zero into an inversion.
#if !defined(DEVOPS_PAIRING)
#define DEVOPS_PAIRING 1
#endif
#define DEVOP_PAIRING(ID, NAME, INW, OUTW) DEVOP_IF(DEVOPS_PAIRING != 0, ID, NAME, INW, OUTW)
using PR = g16::Pairing;
FF_HD g16::fp12_t ld12(const uint32_t* in) { return ldw<g16::fp12_t>(in); }

// (a, b) -> mul(a, b), mul(b, a)
DEVOP_PAIRING(36, "f12_mul", 192, 192) {
  const g16::fp12_t a = ld12(in), b = ld12(in + 96);
  g16::fp12_t r;
  PR::mul(r, a, b);
  stw(out, r);
  PR::mul(r, b, a);
  stw(out + 96, r);
} DEVOP_END
// a -> sqr in place (as the Miller loop and pow_u64 call it), mul(a, a)
DEVOP_PAIRING(37, "f12_sqr", 96, 192) {
  const g16::fp12_t a = ld12(in);
  g16::fp12_t r = a;
  PR::sqr(r, r);
  stw(out, r);
  PR::mul(r, a, a);
  stw(out + 96, r);
} DEVOP_END
// (f, l0 in Fp, l1, l3 in Fp2) -> f * (l0 + l1 w + l3 w^3)
DEVOP_PAIRING(38, "f12_mul_line", 96 + 8 + 16 + 16, 96) {
  g16::fp12_t f = ld12(in);
  PR::mul_line(f, ldw<g16::u256>(in + 96), ldw<g16::fp2_t>(in + 104), ldw<g16::fp2_t>(in + 120));
  stw(out, f);
} DEVOP_END
// a -> conj(a), frobenius(a, 1), frobenius(a, 2), frobenius(a, 3)
DEVOP_PAIRING(39, "f12_frob", 96, 4 * 96) {
  const g16::fp12_t a = ld12(in);
  g16::fp12_t r = a;
  PR::conj(r);
  stw(out, r);
  for (int n = 1; n <= 3; ++n) {
    r = a;
    PR::frobenius(r, n);
    stw(out + 96 * n, r);
  }
} DEVOP_END
DEVOP_PAIRING(40, "f6_mul", 96, 48) {
  g16::fp6_t r;
  PR::f6mul(r, ldw<g16::fp6_t>(in), ldw<g16::fp6_t>(in + 48));
  stw(out, r);
} DEVOP_END
DEVOP_PAIRING(41, "f6_inv", 48, 48) {   // a != 0
  g16::fp6_t r;
  PR::f6inv(r, ldw<g16::fp6_t>(in));
  stw(out, r);
} DEVOP_END
DEVOP_PAIRING(42, "f12_inv", 96, 96) {   // a != 0
  g16::fp12_t r;
  PR::inv(r, ld12(in));
  stw(out, r);
} DEVOP_END
// (a, e: low word, high word) -> a^e
DEVOP_PAIRING(43, "f12_pow_u64", 96 + 2, 96) {
  g16::fp12_t r;
  PR::pow_u64(r, ld12(in), (uint64_t)in[96] | ((uint64_t)in[97] << 32));
  stw(out, r);
} DEVOP_END
// a -> a^6, a^12, a^18, a^30, a^36
DEVOP_PAIRING(44, "f12_small_pows", 96, 5 * 96) {
  PR::Pows p;
  PR::small_pows(p, ld12(in));
  stw(out, p.p6);
  stw(out + 96, p.p12);
  stw(out + 192, p.p18);
  stw(out + 288, p.p30);
  stw(out + 384, p.p36);
} DEVOP_END
DEVOP_PAIRING(45, "f12_is_one", 96, 1) { out[0] = PR::is_one(ld12(in)) ? 1u : 0u; } DEVOP_END
// (P affine in G1, Q affine on the twist) -> the Miller value f_{6x^2,Q}(P), before the final exponentiation
DEVOP_PAIRING(46, "pair_miller", 16 + 32, 96) {
  g16::fp12_t f;
  PR::miller(f, ldw<g16::g1_aff>(in), ldw<g16::g2_aff>(in + 16));
  stw(out, f);
} DEVOP_END
DEVOP_PAIRING(47, "pair_final_exp", 96, 96) {   // f != 0
  g16::fp12_t r;
  PR::final_exp(r, ld12(in));
  stw(out, r);
} DEVOP_END
#undef DEVOP_PAIRING

#if defined(__HIPCC__) && defined(DEVOPS_WITH_MSM)
// ---- msm_digits (msm.cuh; device only) ------------------------------------------------------------------------------
// in: c, mtab, scalars_mont, pad, scalar.  out: count, then per digit  neg << 31 | window (+ selector * nwin) << 24 | bucket
DEVOP(48, "msm_digits", 12, 64) {
#if defined(__HIP_DEVICE_COMPILE__)
  g16::MsmParams P{};
  P.n = 1;
  P.c = in[0];
  P.nwin = g16::FR_BITS / P.c + 1;
  P.mtab = in[1];
  P.scalars_mont = in[2];
  P.tables = 1;
  const g16::u256 s = ldw<g16::u256>(in + 4);
  uint32_t cnt = 0;
  g16::msm_digits(&s, nullptr, 0u, P, [&](uint32_t w, uint32_t k, uint32_t neg) {
    if (cnt < 63) out[1 + cnt] = (neg << 31) | (w << 24) | k;
    ++cnt;
  });
  out[0] = cnt;
#else
  (void)in;
  out[0] = 0;
#endif
} DEVOP_END
constexpr int NOPS = 49;
#else
constexpr int NOPS = 48;
#endif

#undef DEVOP
#undef DEVOP_IF
#undef DEVOP_END

// op -> (name, words in, words out) and the call itself, by linear template recursion
template <int OP = 0>
inline bool info(int op, const char*& name, uint32_t& inw, uint32_t& outw) {
  if (op == OP) {
    name = Op<OP>::name();
    inw = Op<OP>::in_words;
    outw = Op<OP>::out_words;
    return true;
  }
  if constexpr (OP + 1 < NOPS) return info<OP + 1>(op, name, inw, outw);
  return false;
}
// whether this build runs the op
template <int OP = 0>
inline bool carries(int op) {
  if (op == OP) return Op<OP>::carried;
  if constexpr (OP + 1 < NOPS) return carries<OP + 1>(op);
  return false;
}

}  // namespace devops
