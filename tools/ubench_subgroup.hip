// Micro-benchmark of the key audit's order-r pass over an array of G2 points: the library's kernel (audit.cuh: the
// fixed double / add schedule of subgroup_plan.hpp) beside the SAME pass -- canonical check, curve check, [r]Q -- with
// the generic double-and-add ladder the verifier uses for a handful of points (scalar_mul in pairing.hip: a branch per
// scalar bit).  A variant of the benchmark, not of the product: the library never instantiates the generic pass.
//
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 -Iinclude tools/ubench_subgroup.hip -Lnim_groth16_amd/csrc -lg16hip
//         -Wl,-rpath,$PWD/nim_groth16_amd/csrc -o tools/ubench_subgroup
//   tools/ubench_subgroup [log2n = 20] [rounds = 5]
//
// The points are multiples of gen2 by random scalars (g16_fixed_base_g2), so every lane runs the whole ladder and ends in
// the opposite-operands addition.  The two kernels alternate, after one warm-up launch each; times are HIP events
// around single launches; both must report no finding.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../include/g16hip.h"
#include "../nim_groth16_amd/csrc/audit.cuh"

using namespace g16;

#define CHECK(x)                                                                      \
  do {                                                                                \
    hipError_t e__ = (x);                                                             \
    if (e__ != hipSuccess) {                                                          \
      fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e__));                        \
      exit(1);                                                                        \
    }                                                                                 \
  } while (0)

// k * P by double-and-add over the 254 bits of a canonical scalar: the ladder of pairing.hip, word for word
template <class C>
__device__ typename C::Acc scalar_mul(const typename C::Aff& p, u256 k) {
  typename C::Acc acc = C::acc_inf();
#pragma unroll 1
  for (int j = 7; j >= 0; --j) {
    uint32_t limb = k.v[7];
#pragma unroll
    for (int q = 7; q > 0; --q) k.v[q] = k.v[q - 1];   // rotate: static register indices
    k.v[0] = limb;
#pragma unroll 1
    for (int b = 31; b >= 0; --b) {
      acc = C::dbl(acc);
      if ((limb >> b) & 1) C::madd(acc, p);
    }
  }
  return acc;
}
struct GenericLadder {
  __device__ bool operator()(const g2_aff& q) const {
    u256 r{{FrParams::P0, FrParams::P1, FrParams::P2, FrParams::P3, FrParams::P4, FrParams::P5, FrParams::P6,
            FrParams::P7}};
    return G2::is_inf(scalar_mul<G2>(q, r));
  }
};
// WAVES per SIMD asked of the compiler: at 2 (the library kernel's occupancy) hipcc spills 84 bytes per lane of this
// loop, at 1 it keeps everything in 276 registers; both are timed and the faster one is the yardstick
template <int WAVES>
__global__ void __launch_bounds__(AUDIT_BLOCK, WAVES) audit_points_generic(const g2_aff* __restrict__ pts, uint32_t n,
                                                                                  fp2_t b, AuditCounts* __restrict__ out) {
  const uint32_t i = blockIdx.x * AUDIT_BLOCK + threadIdx.x;
  if (i >= n) return;
  const g2_aff p = pts[i];
  const int bad = audit_element<G2, 2>(p, b, nullptr, GenericLadder{});
  if (bad < 0) return;
  atomicMin(&out->first_bad[bad], i);
  atomicAdd(&out->bad_count[bad], 1u);
}

int main(int argc, char** argv) {
  const int log2n = argc > 1 ? atoi(argv[1]) : 20, rounds = argc > 2 ? atoi(argv[2]) : 5;
  if (log2n < 0 || log2n > 24 || rounds < 1) {
    fprintf(stderr, "usage: ubench_subgroup [log2n <= 24] [rounds]\n");
    return 1;
  }
  const size_t n = size_t(1) << log2n;
  g16_ctx* ctx = nullptr;
  if (g16_ctx_create(0, &ctx) != G16_OK) {
    fprintf(stderr, "no usable GPU\n");
    return 1;
  }
  // random scalars below 2^253 (SplitMix64), standard form
  std::vector<uint64_t> sc(4 * n);
  uint64_t state = 20;
  for (auto& w : sc) {
    uint64_t z = (state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    w = z ^ (z >> 31);
  }
  for (size_t i = 0; i < n; ++i) sc[4 * i + 3] &= 0x1fffffffffffffffull;
  std::vector<g2_aff> pts(n);
  if (g16_fixed_base_g2(ctx, sc.data(), G16_SCALARS_STD, n, pts.data()) != G16_OK) {
    fprintf(stderr, "g16_fixed_base_g2: %s\n", g16_last_error(ctx));
    return 1;
  }
  // the twist's b from a point of it: b = y^2 - x^3
  const fp2_t b = Fp2::sub(Fp2::sqr(pts[0].y), Fp2::mul(Fp2::sqr(pts[0].x), pts[0].x));
  g2_aff* d_pts;
  AuditCounts* d_counts;
  CHECK(hipMalloc(&d_pts, n * sizeof(g2_aff)));
  CHECK(hipMalloc(&d_counts, 3 * sizeof(AuditCounts)));
  CHECK(hipMemcpy(d_pts, pts.data(), n * sizeof(g2_aff), hipMemcpyHostToDevice));
  AuditCounts h[3];
  for (auto& c : h)
    for (int k = 0; k < 3; ++k) c.first_bad[k] = 0xffffffffu, c.bad_count[k] = 0;
  CHECK(hipMemcpy(d_counts, h, sizeof h, hipMemcpyHostToDevice));
  hipEvent_t e0, e1;
  CHECK(hipEventCreate(&e0));
  CHECK(hipEventCreate(&e1));
  const uint32_t grid = (uint32_t)((n + AUDIT_BLOCK - 1) / AUDIT_BLOCK);
  auto run = [&](int which) {
    CHECK(hipEventRecord(e0));
    if (which == 0)
      hipLaunchKernelGGL((audit_points<G2, 1>), dim3(grid), dim3(AUDIT_BLOCK), AUDIT_Q_WORDS * AUDIT_BLOCK * 4, 0,
                         (const g2_aff*)d_pts, (uint32_t)n, b, d_counts);
    else if (which == 1)
      hipLaunchKernelGGL(audit_points_generic<2>, dim3(grid), dim3(AUDIT_BLOCK), 0, 0, (const g2_aff*)d_pts, (uint32_t)n, b,
                         d_counts + 1);
    else
      hipLaunchKernelGGL(audit_points_generic<1>, dim3(grid), dim3(AUDIT_BLOCK), 0, 0, (const g2_aff*)d_pts, (uint32_t)n, b,
                         d_counts + 2);
    CHECK(hipGetLastError());
    CHECK(hipEventRecord(e1));
    CHECK(hipEventSynchronize(e1));
    float ms = 0;
    CHECK(hipEventElapsedTime(&ms, e0, e1));
    return (double)ms;
  };
  run(0), run(1), run(2);   // warm-up: code objects loaded
  std::vector<double> t[3];
  for (int r = 0; r < rounds; ++r)
    for (int w = 0; w < 3; ++w) t[w].push_back(run(w));
  CHECK(hipMemcpy(h, d_counts, sizeof h, hipMemcpyDeviceToHost));
  for (int w = 0; w < 3; ++w)
    for (int k = 0; k < 3; ++k)
      if (h[w].bad_count[k]) {
        fprintf(stderr, "%s ladder reports %u findings under check %d on honest points\n", w ? "generic" : "fixed",
                h[w].bad_count[k], k);
        return 1;
      }
  const char* name[3] = {"fixed schedule (audit_points<G2>, the library's kernel)",
                         "generic ladder (scalar_mul<G2> of pairing.hip), 2 waves",
                         "generic ladder (scalar_mul<G2> of pairing.hip), 1 wave"};
  double med[3];
  for (int w = 0; w < 3; ++w) {
    std::sort(t[w].begin(), t[w].end());
    med[w] = t[w][t[w].size() / 2];
    printf("%-58s 2^%d points: median %9.3f ms (min %9.3f, max %9.3f, %d launches) = %7.1f ns per point\n", name[w], log2n,
           med[w], t[w].front(), t[w].back(), rounds, med[w] * 1e6 / (double)n);
  }
  const double gen = std::min(med[1], med[2]);
  printf("fixed / generic (the faster of the two) = %.3f  (condition: the fixed schedule is not slower: %s)\n", med[0] / gen,
         med[0] <= gen ? "met" : "NOT met");
  CHECK(hipFree(d_pts));
  CHECK(hipFree(d_counts));
  g16_ctx_destroy(ctx);
  return 0;
}
