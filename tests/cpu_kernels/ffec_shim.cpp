// Test-only: compiles the *device* field/curve headers with g++ so their formulas can be checked
// against the oracle on a machine without a GPU.  Not part of the product library.
#include "../../nim_groth16_amd/csrc/ec29.cuh"
#include "../../nim_groth16_amd/csrc/pairing.cuh"
#include "../../nim_groth16_amd/csrc/msm_params.hpp"
#include "../../nim_groth16_amd/csrc/msm_plan.hpp"
#include "../../nim_groth16_amd/csrc/spmv_params.hpp"
#include "../../nim_groth16_amd/csrc/ntt_plan.hpp"
#include "../../nim_groth16_amd/csrc/proof_plan.hpp"
#include <cstring>
#include <vector>
using namespace g16;

template <class T> static T ld(const void* p) { T t; std::memcpy(&t, p, sizeof(T)); return t; }
template <class T> static void st(void* p, const T& t) { std::memcpy(p, &t, sizeof(T)); }

// the reduced-radix accumulate path (ec29.cuh): op 0: acc += q_i ; op 1: acc += -(-q_i) through the sign flag
template <class C>
static void sum29(int op, const void* pts, int n, void* out) {
  using E = Ec29<C>;
  typename E::Acc acc = E::acc_inf();
  const char* p = (const char*)pts;
  for (int i = 0; i < n; ++i) {
    typename C::Aff q = ld<typename C::Aff>(p + sizeof(typename C::Aff) * i);
    if (op == 1) q = C::neg(q);
    const typename E::Tab t = E::tab_from_std(q);   // through the packed table entry
    E::madd(acc, &t, op == 1 ? 1u : 0u);
  }
  st(out, C::to_affine(E::to_std(acc)));
}

// op 2: general XYZZ += XYZZ additions in the reduced-radix field: ((q0 + q1) + (q2 + q3)) + ... pairwise tree, so that
// both operands are genuine accumulators
template <class C>
static void tree29(const void* pts, int n, void* out) {
  using E = Ec29<C>;
  std::vector<typename E::Acc> v;
  const char* p = (const char*)pts;
  for (int i = 0; i < n; ++i) {
    typename E::Acc a = E::acc_inf();
    const typename E::Tab t = E::tab_from_std(ld<typename C::Aff>(p + sizeof(typename C::Aff) * i));
    E::madd(a, &t, 0u);
    v.push_back(a);
  }
  while (v.size() > 1) {
    std::vector<typename E::Acc> w;
    for (size_t i = 0; i + 1 < v.size(); i += 2) {
      typename E::Acc a = v[i];
      E::add(a, v[i + 1]);
      w.push_back(a);
    }
    if (v.size() & 1) w.push_back(v.back());
    v.swap(w);
  }
  st(out, C::to_affine(v.empty() ? C::acc_inf() : E::to_std(v[0])));
}

extern "C" {
// bs_block (msm_params.hpp): every (partition, slice) exactly once, and all slices of a partition on one XCD (same
// block index modulo 8) whenever the partition count is a multiple of 8.  -> 0 if so
uint32_t shim_bs_block_check(uint32_t nparts) {
  std::vector<uint8_t> seen((size_t)nparts * BS_SPLIT, 0);
  std::vector<int> xcd(nparts, -1);
  for (uint32_t b = 0; b < nparts * BS_SPLIT; ++b) {
    uint32_t part = ~0u, q = ~0u;
    bs_block(b, nparts, part, q);
    if (part >= nparts || q >= (uint32_t)BS_SPLIT || seen[(size_t)part * BS_SPLIT + q]++) return 1 + b;
    if ((nparts & 7u) == 0) {
      if (xcd[part] < 0) xcd[part] = (int)(b & 7u);
      else if (xcd[part] != (int)(b & 7u)) return 1 + b;
    }
  }
  return 0;
}

// the row bins of the row-balanced sparse kernel (spmv_params.hpp): -> 0, or 1 + the first row length that breaks a rule
uint32_t shim_spmv_bins_check(uint32_t max_len) {
  uint32_t prev = 0;
  for (uint32_t L = 0; L <= max_len; ++L) {
    const uint32_t b = bin_of(L);
    if (b >= (uint32_t)NBINS || b < prev) return 1 + L;                       // monotone in L
    prev = b;
    const uint32_t lanes = 1u << bin_glog(b), per_trip = bin_terms(b) * lanes;
    if (lanes > 64 || (BLOCK % lanes) != 0) return 1 + L;
    if (b + 1 < (uint32_t)NBINS && L > per_trip) return 1 + L;               // one trip everywhere but in the last bin
    if (b >= 3 && L <= per_trip / 2) return 1 + L;                           // groups are at least half full
    if (b == 0 && L > 1) return 1 + L;
    if (b == 1 && L != 2) return 1 + L;
    if (b == 2 && (L < 3 || L > 4)) return 1 + L;
  }
  return 0;
}

// the NTT pass plan of geometry `tile` (ntt_plan.hpp) at 2^log2n: geometry {log2tile, max_rho, opt-in LDS, one-pass},
// then per pass {rho, log2b, log2s, ntiles, shmem} into out[4 + 5 p ..].  -> npass
uint32_t shim_ntt_plan(int tile, uint32_t log2n, uint64_t* out) {
  const NttGeom g = ntt_geom(tile);
  const uint32_t npass = ntt_npass(g, log2n);
  out[0] = g.log2tile;
  out[1] = g.max_rho;
  out[2] = ntt_optin_shmem();
  out[3] = ntt_one_pass(g, log2n) ? 1 : 0;
  for (uint32_t p = 0; p < npass; ++p) {
    const NttPass q = ntt_pass_plan(g, log2n, p);
    uint64_t* o = out + 4 + 5 * p;
    o[0] = q.rho;
    o[1] = q.log2b;
    o[2] = q.log2s;
    o[3] = q.ntiles;
    o[4] = q.shmem;
  }
  return npass;
}

// The MSM launch plan (msm_plan.hpp) of n pairs.  table_cfg 0: a plain MSM, 1: a registered set (window and multiplier
// tables chosen as registration does).  knobs: {msm_window, table_window, msm_seg, msm_sort, red_slice_log2, r2_width,
// mtab, tail_quad, red_chunk, heavy_grid} as G16Env holds them.  out:
//   [0..8]   MsmParams  n c nwin nbuckets seg scalars_mont tables max_extra mtab
//   [9..18]  sort plan  lo_bits nparts ptiles nth use_part fused nblk ntiles nt2 pblk
//   [19..35] offsets of the 16 parts of the sort workspace, in order, and its size
//   [36..45] G1 then G2: offsets of the 4 parts of a job workspace and its size
//   [46..56] tail plan  rc nchunks nsets log2ks cps r2 r2_threads r2_lds fold heavy_grid(1) heavy_grid(3)
// The mirrors of g16_ctx::MsmSort / MsmJob hold the parts as bytes; the carver runs over a base that is never touched.
struct ShimSortParts {
  char *count, *cursor, *offset, *xoff, *heavy, *info, *tiles, *entries, *xseg, *perm, *ghist, *blk_base, *tile_hist, *tmp,
      *tiles2, *slice_hist;
};
struct ShimJobParts {
  char *partial, *chunkR, *chunkA, *wsum;
};
static G16Env shim_env(const int* knobs) {
  G16Env env;
  env.msm_window = knobs[0];
  env.table_window = knobs[1];
  env.msm_seg = knobs[2];
  env.msm_sort = (char)knobs[3];
  env.red_slice_log2 = knobs[4];
  env.r2_width = knobs[5];
  env.mtab = knobs[6];
  env.tail_quad = knobs[7];
  env.red_chunk = knobs[8];
  env.heavy_grid = knobs[9];
  return env;
}
static void shim_tail_out(const MsmTailPlan& T, uint64_t* out) {
  const uint64_t t[11] = {T.rc, T.nchunks, T.nsets, T.log2ks, T.cps, (uint64_t)T.r2, T.r2_threads, T.r2_lds, (uint64_t)T.fold,
                          T.heavy_grid(1), T.heavy_grid(3)};
  for (int i = 0; i < 11; ++i) out[i] = t[i];
}
// the tail plan alone, of parameters given field by field (the order of out[0..8] below): bucket sets that no point
// count produces, such as one of 511 chunks
void shim_msm_tail_plan(const uint32_t* p, int is_g1, int narrow_tail, const int* knobs, uint64_t* out) {
  MsmParams P;
  P.n = p[0], P.c = p[1], P.nwin = p[2], P.nbuckets = p[3], P.seg = p[4], P.scalars_mont = p[5], P.tables = p[6];
  P.max_extra = p[7], P.mtab = p[8];
  shim_tail_out(msm_tail_plan(P, is_g1 != 0, narrow_tail != 0, shim_env(knobs)), out);
}
void shim_msm_plan(uint64_t n, uint32_t flags, int table_cfg, int is_g1, int narrow_tail, const int* knobs, uint64_t* out) {
  const G16Env env = shim_env(knobs);
  uint32_t cfg = 0;
  if (table_cfg) {
    const uint32_t c = msm_pick_table_window(n, env);
    cfg = c | (msm_pick_mtab(c, env) << 8);
  }
  const MsmParams P = msm_params(n, flags, cfg, env);
  const uint32_t p[9] = {P.n, P.c, P.nwin, P.nbuckets, P.seg, P.scalars_mont, P.tables, P.max_extra, P.mtab};
  for (int i = 0; i < 9; ++i) out[i] = p[i];
  const MsmSortPlan L = msm_sort_plan(P, env);
  const uint64_t l[10] = {L.lo_bits, L.nparts, L.ptiles, L.nth, L.use_part, L.fused, L.nblk, L.ntiles, L.nt2, L.pblk};
  for (int i = 0; i < 10; ++i) out[9 + i] = l[i];
  char* const base = reinterpret_cast<char*>(uintptr_t(1) << 40);
  ShimSortParts S;
  Carver sort{base};
  msm_sort_layout(S, P, L, sort);
  char* const sp[16] = {S.count, S.cursor, S.offset, S.xoff, S.heavy, S.info, S.tiles, S.entries, S.xseg, S.perm, S.ghist,
                        S.blk_base, S.tile_hist, S.tmp, S.tiles2, S.slice_hist};
  for (int i = 0; i < 16; ++i) out[19 + i] = (uint64_t)(sp[i] - base);
  Carver sort_size{nullptr};
  msm_sort_layout(S, P, L, sort_size);
  out[35] = sort_size.bytes;
  const MsmTailPlan T = msm_tail_plan(P, is_g1 != 0, narrow_tail != 0, env);
  for (int g = 0; g < 2; ++g) {
    ShimJobParts J;
    Carver job{base}, job_size{nullptr};
    msm_job_layout(J, P, T.nchunks, g ? 256 : 128, g ? 288 : 144, job);
    char* const jp[4] = {J.partial, J.chunkR, J.chunkA, J.wsum};
    for (int i = 0; i < 4; ++i) out[36 + 5 * g + i] = (uint64_t)(jp[i] - base);
    msm_job_layout(J, P, T.nchunks, g ? 256 : 128, g ? 288 : 144, job_size);
    out[40 + 5 * g] = job_size.bytes;
  }
  shim_tail_out(T, out + 46);
}

// The launch schedule of a proof (proof_plan.hpp).  knobs: {quotient_first, lanes_after_quotient, g1_batch, chain_ch,
// cu_split, cz_on_the_fly, g2_first, g1_lanes[3]} as G16Env holds them; shape: {nw, nh, log2n, liveA, liveB, cfg_equal}.
// out: {fits, count, narrow_tail, sort_a, sort_b}, then {op, stream, a, b, c, d, e} per step.  -> count
int shim_proof_plan(const int* knobs, int entry, uint32_t task_mask, int host_sync, const uint64_t* shape, int cap,
                    int32_t* out) {
  G16Env env;
  env.quotient_first = knobs[0], env.lanes_after_quotient = knobs[1], env.g1_batch = knobs[2], env.chain_ch = knobs[3];
  env.cu_split = knobs[4], env.cz_on_the_fly = knobs[5], env.g2_first = knobs[6];
  for (int i = 0; i < 3; ++i) env.g1_lanes[i] = knobs[7 + i];
  const ProofShape s{(size_t)shape[0], (size_t)shape[1], (uint32_t)shape[2], shape[3] != 0, shape[4] != 0, shape[5] != 0};
  ProofPlan p;
  out[0] = proof_plan_build(p, env, (ProofEntry)entry, task_mask, host_sync != 0, s, cap) ? 1 : 0;
  out[1] = p.count, out[2] = p.narrow_tail, out[3] = p.sort_a, out[4] = p.sort_b;
  for (int i = 0; i < p.count; ++i) {
    const ProofStep& t = p.steps[i];
    const int32_t v[7] = {t.op, t.stream, t.a, t.b, t.c, t.d, t.e};
    for (int j = 0; j < 7; ++j) out[5 + 7 * i + j] = v[j];
  }
  return p.count;
}
// the helpers next to it: the sparsity predicate at G16_INF_COMPACT = pct, the CU mask at G16_CU_SPLIT = k, the
// priority of stream `index` under G16_STREAM_PRIO = cfg (six characters)
int shim_points_sparse(uint64_t n_inf, uint64_t n, int pct) {
  G16Env env;
  env.inf_compact_pct = pct;
  return points_sparse(n_inf, n, env) ? 1 : 0;
}
void shim_cu_mask(int k, int front, uint32_t* mask) {
  G16Env env;
  env.cu_split = k;
  stream_cu_mask(env, front != 0, mask);
}
int shim_stream_priority(const char* cfg, int index, int lo, int hi) {
  G16Env env;
  memcpy(env.stream_prio, cfg, 6);
  return stream_priority(env, index, lo, hi);
}

// the class bucket set of registered point sets with two multiplier tables (msm_params.hpp): every digit magnitude
// t in [1, 2^(c-1)] must land in a bucket whose weight (from the class layout, restated here) times 2^s is t, every
// bucket must be hit once or twice, and none may lie outside the set.  -> 0, or the first offending t
uint32_t shim_class_buckets_check(uint32_t c) {
  const uint32_t h = 1u << (c - 1), nb = msm_table_buckets(c, 2);
  std::vector<uint8_t> hits(nb, 0);
  auto weight = [&](uint32_t id) -> uint64_t {
    if (id < h / 2) return 2ull * id + 1;
    if (id < h / 2 + h / 8) return 4ull * (2ull * (id - h / 2) + 1);
    if (id < h / 2 + h / 8 + h / 32) return 16ull * (2ull * (id - h / 2 - h / 8) + 1);
    return 64ull * (id - h / 2 - h / 8 - h / 32 + 1);
  };
  for (uint32_t t = 1; t <= h; ++t) {
    uint32_t s = 9;
    const uint32_t id = msm_class_bucket(t, c, s);
    if (id >= nb || s > 1 || (weight(id) << s) != t) return t;
    if (++hits[id] > 2) return t;
  }
  for (uint32_t id = 0; id < nb; ++id)
    if (!hits[id]) return 0x80000000u | id;
  return nb == h / 2 + h / 8 + h / 32 + h / 64 && nb % (MSM_CLASS_SLICES) == 0 && nb / MSM_CLASS_SLICES == (1u << (c - 7)) ? 0 : 1;
}

// msm_class_slice (msm_params.hpp) as the class folds read it -> out[5] = z, first, end, doublings of y_v, of e_v
void shim_class_slice(int v, int32_t* out) {
  const MsmClassSlice s = msm_class_slice(v);
  out[0] = s.z, out[1] = s.first, out[2] = s.end, out[3] = s.dbl_y, out[4] = s.dbl_e;
}

// op: 0 add 1 sub 2 mul 3 sqr 4 neg 5 dbl 6 div2 7 inv 8 from_mont 9 to_mont ; field: 0 Fp 1 Fr
void shim_field_op(int field, int op, const void* a, const void* b, void* r) {
  u256 x = ld<u256>(a), y = ld<u256>(b), z;
  auto run = [&](auto F) {
    using FF = decltype(F);
    switch (op) {
      case 0: z = FF::add(x, y); break;
      case 1: z = FF::sub(x, y); break;
      case 2: z = FF::mul(x, y); break;
      case 3: z = FF::sqr(x); break;
      case 4: z = FF::neg(x); break;
      case 5: z = FF::dbl(x); break;
      case 6: z = FF::div2(x); break;
      case 7: z = FF::inv(x); break;
      case 8: z = FF::from_mont(x); break;
      default: z = FF::to_mont(x); break;
    }
  };
  if (field == 0) run(Fp{}); else run(Fr{});
  st(r, z);
}
// op: 0 add 1 sub 2 mul 3 sqr 4 neg 7 inv
void shim_fp2_op(int op, const void* a, const void* b, void* r) {
  fp2_t x = ld<fp2_t>(a), y = ld<fp2_t>(b), z;
  switch (op) {
    case 0: z = Fp2::add(x, y); break;
    case 1: z = Fp2::sub(x, y); break;
    case 2: z = Fp2::mul(x, y); break;
    case 3: z = Fp2::sqr(x); break;
    case 4: z = Fp2::neg(x); break;
    default: z = Fp2::inv(x); break;
  }
  st(r, z);
}
// sums n affine points with madd (op 0), or with XYZZ+XYZZ add of from_affine (op 1), or as
// k*P via mul_small on the first point (op 2, k = n); returns the canonical affine result
void shim_g1_sum(int op, const void* pts, int n, void* out) {
  g1_acc acc = G1::acc_inf();
  const char* p = (const char*)pts;
  if (op == 2) {
    acc = G1::mul_small(G1::from_affine(ld<g1_aff>(p)), (uint32_t)n);
  } else {
    for (int i = 0; i < n; ++i) {
      g1_aff q = ld<g1_aff>(p + 64 * i);
      if (op == 0) G1::madd(acc, q); else G1::add(acc, G1::from_affine(q));
    }
  }
  st(out, G1::to_affine(acc));
}
void shim_g1_sum29(int op, const void* pts, int n, void* out) { if (op == 2) tree29<G1>(pts, n, out); else sum29<G1>(op, pts, n, out); }
void shim_g2_sum29(int op, const void* pts, int n, void* out) { if (op == 2) tree29<G2>(pts, n, out); else sum29<G2>(op, pts, n, out); }
// op 0: to_std(mul(from_std a, from_std b))  1: to_std(sqr(from_std a))  2: to_std(from_std a)
// 3: to_std(dot2(a,b,a,b)) = 2ab
void shim_f29_op(int op, const void* a, const void* b, void* r) {
  fe29 x = Fp29::from_std(ld<u256>(a)), y = Fp29::from_std(ld<u256>(b)), z;
  switch (op) {
    case 0: z = Fp29::mul(x, y); break;
    case 1: z = Fp29::sqr(x); break;
    case 2: z = x; break;
    default: z = Fp29::dot2(x, y, x, y); break;
  }
  st(r, Fp29::to_std(z));
}
void shim_g2_sum(int op, const void* pts, int n, void* out) {
  g2_acc acc = G2::acc_inf();
  const char* p = (const char*)pts;
  if (op == 2) {
    acc = G2::mul_small(G2::from_affine(ld<g2_aff>(p)), (uint32_t)n);
  } else {
    for (int i = 0; i < n; ++i) {
      g2_aff q = ld<g2_aff>(p + 128 * i);
      if (op == 0) G2::madd(acc, q); else G2::add(acc, G2::from_affine(q));
    }
  }
  st(out, G2::to_affine(acc));
}
// op 0: Miller loop f_{6x^2,Q}(P)   1: full pairing   2: final exponentiation of the Fp12 element at `p`
// out: 6 x Fp2 (384 bytes, Montgomery form), coefficient k belongs to w^k
void shim_pairing(int op, const void* p, const void* q, void* out) {
  fp12_t f;
  if (op == 2) {
    Pairing::final_exp(f, ld<fp12_t>(p));
  } else {
    Pairing::miller(f, ld<g1_aff>(p), ld<g2_aff>(q));
    if (op == 1) { fp12_t t = f; Pairing::final_exp(f, t); }
  }
  st(out, f);
}
}
