// Parameters of one MSM launch sequence (shared by host and device code).
#pragma once
#include <stdint.h>

namespace g16 {
struct MsmParams {
  uint32_t n;            // number of (scalar, point) pairs
  uint32_t c;            // window bits
  uint32_t nwin;         // number of windows  = 254 / c + 1
  uint32_t nbuckets;     // tables: 1 << (c-1) (ONE bucket set shared by all windows; tstride << (c-1) for a lean set); else nwin << (c-1)
  uint32_t seg;          // L: max entries per accumulate task
  uint32_t scalars_mont; // 1: scalars are Montgomery Fr limbs (Nim seq[Fr]); 0: canonical LE (.wtns)
  uint32_t tables;       // 1: points array holds nwin tables [w][i] = 2^(c w) P_i (registered point set);
                         //    the 2^(c w) factor lives in the table, so every window uses the same buckets
  uint32_t max_extra;    // capacity of the extra-segment list
  uint32_t mtab;         // multiplier tables per window (registered sets): 1, or 2 = {1, 2} -- the points array then
                         //    holds tables [m][w][i] = 2^(c w + m) P_i and the bucket set is the CLASS set of msm.cuh
                         //    (msm_class_bucket): 0.67 x the buckets for the same windows
  uint32_t tstride = 0;  // table stride s of a registered set: a table for every s-th window, [j][i] = 2^(c s j) P_i, and
                         //    window w = s j + r gathers from table j into bucket set r (msm_window_slot).  0: no tables,
                         //    1: a table per window (one bucket set; `tables`, `mtab` as above), >= 2: a lean set --
                         //    ceil(nwin / s) tables, s bucket sets of 2^(c-1) buckets, mtab = 1
};
// number of buckets of a merged (registered) bucket set
inline uint32_t msm_table_buckets(uint32_t c, uint32_t mtab) {
  const uint32_t h = 1u << (c - 1);
  return mtab == 2 ? h / 2 + h / 8 + h / 32 + h / 64 : h;   // classes b = 4^z u (z = 0, 1, 2; u odd) + the 64 x class
}
constexpr uint32_t MSM_CLASS_SLICES = 32 + 8 + 2 + 1;   // slices of 2^(c-7) buckets: class 0, 1, 2, X
#if defined(__HIPCC__)
#define G16_MSMP_HD __host__ __device__ __forceinline__
#else
#define G16_MSMP_HD inline
#endif

// ---- launch geometry that the kernels (msm.cuh) and the host sizing (msm_plan.hpp) both use ------------------------
constexpr int MSM_BLOCK = 256;
constexpr int FR_BITS = 254;
// 1024 threads x 4 scalars: the pass is a chain of dependent LDS atomics and scattered 8-byte stores per thread, and a
// 2^20-scalar sort has only 256 tiles -- one workgroup per CU -- so the workgroup is as wide as it gets (16 waves per
// CU hide that latency; rounds 1-2 ran 256 threads x 16 scalars = ONE wave per SIMD)
// Low bucket bits sorted inside a partition (bucket_hist / bucket_place: one thread per low value).  Round 4: 9 instead
// of 8 -- half as many partitions (688 for the class set of c = 20), hence half as many (tile, partition) runs that
// part_pass<true> keeps open at once: 32 tiles per XCD x 1376 runs x one active 128-byte line were 5.6 MB against a
// 4-MB L2, and lines left the L2 half written (WRITE_SIZE 3.4 x the record bytes); 688 runs are 2.8 MB.
constexpr int BS_LOG = 9;
constexpr int BS_LOW = 1 << BS_LOG;
constexpr int PART_BLOCK = 1024;
constexpr int PART_PER_THREAD = 4;
constexpr int PART_TILE = PART_BLOCK * PART_PER_THREAD;  // scalars per workgroup
constexpr int PART_MAX = 8192;                           // max partitions (LDS histogram, 32 KB)
constexpr int PERM_BINS = 256;   // size classes of the bucket-order permutation (perm_hist / perm_scatter, msm.cuh)
constexpr int PERM_BLOCK = BS_LOW;   // = one partition of the fused sort (bucket_place writes blk_base per partition)
// the three-phase exclusive scan over the bucket histogram (msm.cuh)
constexpr int SCAN_BLOCK = 256;
constexpr int SCAN_ITEMS = 8;                       // per thread
constexpr int SCAN_TILE = SCAN_BLOCK * SCAN_ITEMS;  // 2048 buckets per workgroup

// (partition, slice) of workgroup `bid` of bucket_hist / bucket_place; see msm.cuh
constexpr int BS_SPLIT = 8;
G16_MSMP_HD void bs_block(uint32_t bid, uint32_t nparts, uint32_t& part, uint32_t& q) {
  if (BS_SPLIT == 8 && (nparts & 7u) == 0) {
    const uint32_t j = bid >> 3;
    part = ((j >> 3) << 3) | (bid & 7u);
    q = j & 7u;
  } else {
    part = bid / BS_SPLIT;
    q = bid % BS_SPLIT;
  }
}
// window w of a point set stored at table stride s -> (table j, bucket set r), w = s j + r:
//   sum_w 2^(c w) D_w  =  sum_{r < s} 2^(c r) * ( sum_j 2^(c s j) D_{s j + r} ).
// s = 0 (no tables: every window is its own bucket set) and s = 1 (a table per window: one bucket set) are the two ends
// and divide nothing.
G16_MSMP_HD void msm_window_slot(uint32_t w, uint32_t tstride, uint32_t& table, uint32_t& set) {
  if (tstride == 1) {
    table = w;
    set = 0;
  } else if (tstride == 0) {
    table = 0;
    set = w;
  } else {
    table = w / tstride;
    set = w - table * tstride;
  }
}
// digit magnitude t in [1, 2^(c-1)] -> (class bucket, table selector s): t = 2^s * weight(bucket); see msm.cuh
G16_MSMP_HD uint32_t msm_class_bucket(uint32_t t, uint32_t c, uint32_t& s) {
  const uint32_t tz = (uint32_t)__builtin_ctz(t), h = 1u << (c - 1);
  if (tz >= 6) {
    s = 0;
    return h / 2 + h / 8 + h / 32 + (t >> 6) - 1;
  }
  s = tz & 1u;
  const uint32_t z = tz >> 1, v = (t >> (tz + 1));          // t = 2^tz (2 v + 1)
  const uint32_t base = z == 0 ? 0u : z == 1 ? h / 2 : h / 2 + h / 8;
  return base + v;
}
// ---- the digits of a scalar and where they go: ONE definition, for the sort and for the sparse run ---------------------
// Signed c-bit digits of a canonical scalar, least significant window first.  The scalar stays in its 8 words and is
// shifted right by c bits per window (on the device: 8 funnel shifts with static register indices, c <= 22 < 32): no LDS
// staging, no dynamic limb indexing, and any workgroup size.  (Rounds 1-2 staged the limbs in LDS and indexed them by
// window: 36 KB of LDS per 1024 threads and two LDS reads per digit.)  A window value above 2^(c-1), carry included,
// becomes the negative digit value - 2^c with a carry into the next window; digit 0 emits nothing.
//   emit(w + table selector * nwin, bucket, negative)   class bucket set (mtab == 2): the entry then indexes table [s][w]
//   emit(w, magnitude - 1, negative)                    every other set
// `s` is consumed.
template <class EMIT>
G16_MSMP_HD void msm_digit_walk(uint32_t (&s)[8], const MsmParams& P, EMIT&& emit) {
  const uint32_t c = P.c, half = 1u << (c - 1), mask = (1u << c) - 1;
  uint32_t carry = 0;
  for (uint32_t w = 0; w < P.nwin; ++w) {
    uint32_t raw = (s[0] & mask) + carry;
    uint32_t neg = raw > half ? 1u : 0u;
    uint32_t mag = neg ? (1u << c) - raw : raw;
    carry = neg;
    if (mag) {
      if (P.mtab == 2) {
        uint32_t sel;
        const uint32_t b = msm_class_bucket(mag, c, sel);
        emit(w + sel * P.nwin, b, neg);
      } else {
        emit(w, mag - 1, neg);
      }
    }
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
    for (int j = 0; j < 7; ++j) s[j] = __builtin_amdgcn_alignbit(s[j + 1], s[j], c);
#else
    for (int j = 0; j < 7; ++j) s[j] = (s[j] >> c) | (s[j + 1] << (32 - c));
#endif
    s[7] >>= c;
  }
}
// Where the entry of digit (window w, pair i) goes: the offset of its bucket set, in units of 1 << shift buckets, and the
// table-major index of its point.  LEAN: a set with tables at a stride >= 2 (msm_window_slot divides).  The two ends of
// the family -- no tables, a table per window -- divide nothing and keep the expressions they always had; the host picks
// the instantiation (g16_msm_sort).
template <bool LEAN>
G16_MSMP_HD void msm_entry_place(const MsmParams& P, uint32_t w, uint32_t i, uint32_t shift, uint32_t& set_off,
                                 uint32_t& pidx) {
  if (LEAN) {
    uint32_t table, set;
    msm_window_slot(w, P.tstride, table, set);
    set_off = set << shift;
    pidx = table * P.n + i;
  } else {
    set_off = P.tables ? 0u : (w << shift);
    pidx = P.tables ? (w * P.n + i) : i;
  }
}
// The sparse run of a point set with a handful of live points (msm_sparse_accum, msm.cuh) reads no arrangement: it forms
// the entries of its live pairs itself.  A hit is what the sort would have placed for one digit -- the bucket, which is
// also the slot of its sum, and the entry, the table-major point index | sign << 31 -- and the hits of pair i with the
// canonical scalar s (consumed) come out in window order: out has room for P.nwin of them.  -> their number
struct MsmHit {
  uint32_t slot, entry;
};
constexpr uint32_t MSM_HIT_NONE = 0xffffffffu;   // in `slot`: no hit
G16_MSMP_HD uint32_t msm_hit_list(uint32_t (&s)[8], uint32_t i, const MsmParams& P, MsmHit* out) {
  uint32_t k = 0;
  const uint32_t shift = P.c - 1;
  msm_digit_walk(s, P, [&](uint32_t w, uint32_t b, uint32_t neg) {
    uint32_t set_off, pidx;
    if (P.tstride >= 2)
      msm_entry_place<true>(P, w, i, shift, set_off, pidx);
    else
      msm_entry_place<false>(P, w, i, shift, set_off, pidx);
    out[k].slot = set_off + b;
    out[k].entry = pidx | (neg << 31);
    ++k;
  });
  return k;
}

// Slice v of the class set (MSM_CLASS_SLICES slices of 2^(c-7) buckets, in msm_class_bucket's bucket order): its class
// z (0, 1, 2; 3 = X), the slices [first, end) of that class, and the doublings that scale the slice's two terms in the
// fold by 4^z (msm_fold_classes, msm.cuh): y_v = 4^z (2 W_v - T_v) starts from 2 W_v, so that X's 64 W_v takes 5;
// e_v = 4^z sigma, and X has none.  v >= MSM_CLASS_SLICES (an idle lane of a fold) reads as class X.
struct MsmClassSlice {
  int z, first, end, dbl_y, dbl_e;
};
G16_MSMP_HD MsmClassSlice msm_class_slice(int v) {
  const int z = v < 32 ? 0 : v < 40 ? 1 : v < 42 ? 2 : 3;
  const int first = z == 0 ? 0 : z == 1 ? 32 : z == 2 ? 40 : 42;
  const int end = z == 0 ? 32 : z == 1 ? 40 : z == 2 ? 42 : (int)MSM_CLASS_SLICES;
  return MsmClassSlice{z, first, end, z == 0 ? 0 : z == 1 ? 2 : z == 2 ? 4 : 5, z == 1 ? 2 : z == 2 ? 4 : 0};
}
}  // namespace g16
