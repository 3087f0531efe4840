// G1 registration-time tables, fixed-base multiples of gen1, on-curve check; the sparse run of the accumulate stage
// (msm_sparse_accum: built here, in the plain arithmetic configuration, and not beside msm_accum -- msm_g1_accum.o holds
// the one hot loop that the instruction budgets are counted on)
#include "msm_stage.cuh"
template <>
struct CurveConsts<G1> {
  // gen1 = (1, 2)  (curves.nim:112-113)
  static g1_aff gen() { return g1_aff{Fp::one(), Fp::dbl(Fp::one())}; }
  // y^2 = x^3 + 3  (curves.nim:54-67)
  static u256 b() { return Fp::add(Fp::dbl(Fp::one()), Fp::one()); }
};
template int32_t to29_device<G1>(g16_ctx*, hipStream_t, const void*, size_t, void*);
template int32_t precompute_device<G1>(g16_ctx*, const void*, size_t, uint32_t, uint32_t, uint32_t, void*);
template int32_t fixed_base_device<G1>(g16_ctx*, void*, bool, const void*, uint32_t, size_t, void*);
template int32_t on_curve_device<G1>(g16_ctx*, const void*, size_t, uint32_t*);
template int32_t live_bitmap_device<G1>(g16_ctx*, const void*, size_t, uint32_t*, uint32_t*);
template int32_t stage_accum_sparse<G1>(g16_ctx*, hipStream_t, const MsmParams&, const g16_msm_sparse&, const void*, void*,
                                        bool);

// the OR of two live bitmaps looks at no point: it sits here beside the kernel that makes them
int32_t g16_bitmap_or_device(g16_ctx* ctx, uint32_t* d_out, const uint32_t* d_a, const uint32_t* d_b, size_t n,
                             uint32_t* d_n_dead) {
  if (n)
    KLAUNCH(ctx, "bitmap_or", bitmap_or, (uint32_t)(((n + 31) / 32 + 255) / 256), 256, 0, d_out, d_a, d_b, (uint32_t)n,
            d_n_dead);
  HIPCHK(ctx, hipGetLastError());
  return G16_OK;
}
