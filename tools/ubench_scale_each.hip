// Micro-benchmark of a scalar PER POINT times an array of points, two ways in one process on the same points and scalars:
//   plain  the only way before scale_each.cuh existed: cs_term with per-point scalars (the 254-bit ladder of
//          scalar_mul.cuh per lane, XYZZ written to global memory) and then cs_to_affine (one field inversion per
//          point), two launches, the very kernels of circuit_setup.cuh;
//   each   scale_each (scale_each.cuh): G1 splits the lane's scalar through the endomorphism and walks 128 columns, G2
//          the same ladder as `plain`; both one inversion per four points, one launch.
//
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 -Iinclude tools/ubench_scale_each.hip -Lnim_groth16_amd/csrc -lg16hip
//         -Wl,-rpath,$PWD/nim_groth16_amd/csrc -o tools/ubench_scale_each
//   tools/ubench_scale_each [group = 1] [log2n = 20] [rounds = 7]
//
// The points are multiples of the generator by random scalars (g16_fixed_base_g1/g2), the scalars n more random draws
// below 2^253, standard form.  The two paths alternate after one warm-up each; times are HIP events around the launches
// of a path; the outputs must agree byte for byte.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../include/g16hip.h"
#include "../nim_groth16_amd/csrc/circuit_setup.cuh"
#include "../nim_groth16_amd/csrc/scale_each.cuh"

using namespace g16;

#define CHECK(x)                                                                      \
  do {                                                                                \
    hipError_t e__ = (x);                                                             \
    if (e__ != hipSuccess) {                                                          \
      fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e__));                        \
      exit(1);                                                                        \
    }                                                                                 \
  } while (0)

template <class C>
static int bench(g16_ctx* ctx, int group, int log2n, int rounds) {
  using Aff = typename C::Aff;
  using Acc = typename C::Acc;
  const size_t n = size_t(1) << log2n;
  // random scalars below 2^253 (SplitMix64), standard form: n logarithms of the points, then the n multipliers
  std::vector<uint64_t> sc(4 * 2 * n);
  uint64_t state = 21;
  for (auto& w : sc) {
    uint64_t z = (state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    w = z ^ (z >> 31);
  }
  for (size_t i = 0; i < 2 * n; ++i) sc[4 * i + 3] &= 0x1fffffffffffffffull;
  std::vector<Aff> pts(n);
  const int32_t rc = group == 1 ? g16_fixed_base_g1(ctx, sc.data(), G16_SCALARS_STD, n, pts.data())
                                : g16_fixed_base_g2(ctx, sc.data(), G16_SCALARS_STD, n, pts.data());
  if (rc != G16_OK) {
    fprintf(stderr, "g16_fixed_base: %s\n", g16_last_error(ctx));
    return 1;
  }
  Aff *d_pts, *d_out[2];
  Acc* d_work;
  u256* d_k;
  CHECK(hipMalloc(&d_pts, n * sizeof(Aff)));
  CHECK(hipMalloc(&d_out[0], n * sizeof(Aff)));
  CHECK(hipMalloc(&d_out[1], n * sizeof(Aff)));
  CHECK(hipMalloc(&d_work, n * sizeof(Acc)));
  CHECK(hipMalloc(&d_k, n * 32));
  CHECK(hipMemcpy(d_pts, pts.data(), n * sizeof(Aff), hipMemcpyHostToDevice));
  CHECK(hipMemcpy(d_k, sc.data() + 4 * n, n * 32, hipMemcpyHostToDevice));
  hipEvent_t e0, e1;
  CHECK(hipEventCreate(&e0));
  CHECK(hipEventCreate(&e1));
  auto run = [&](int which) {
    CHECK(hipEventRecord(e0));
    if (which == 0) {
      hipLaunchKernelGGL(cs_term<C>, dim3(cs_grid(n)), dim3(CS_BLOCK), 0, 0, (const Aff*)d_pts, (const uint32_t*)nullptr,
                         (const u256*)d_k, (const uint32_t*)nullptr, 1u, 0u, 0u, (uint32_t)n, d_work);
      hipLaunchKernelGGL(cs_to_affine<C>, dim3(cs_grid(n)), dim3(CS_BLOCK), 0, 0, (const Acc*)d_work, (uint32_t)n,
                         d_out[0]);
    } else {
      hipLaunchKernelGGL(scale_each<C>, dim3((uint32_t)((n + SCALE_TILE - 1) / SCALE_TILE)), dim3(SCALE_BLOCK), 0, 0,
                         (const Aff*)d_pts, (const u256*)d_k, 0u, (uint32_t)n, d_out[1]);
    }
    CHECK(hipGetLastError());
    CHECK(hipEventRecord(e1));
    CHECK(hipEventSynchronize(e1));
    float ms = 0;
    CHECK(hipEventElapsedTime(&ms, e0, e1));
    return (double)ms;
  };
  run(0), run(1);   // warm-up: code objects loaded
  std::vector<double> t[2];
  for (int r = 0; r < rounds; ++r)
    for (int w = 0; w < 2; ++w) t[w].push_back(run(w));
  std::vector<Aff> got[2] = {std::vector<Aff>(n), std::vector<Aff>(n)};
  for (int w = 0; w < 2; ++w) CHECK(hipMemcpy(got[w].data(), d_out[w], n * sizeof(Aff), hipMemcpyDeviceToHost));
  if (memcmp(got[0].data(), got[1].data(), n * sizeof(Aff))) {
    fprintf(stderr, "the two paths differ\n");
    return 1;
  }
  const char* name[2] = {"plain (cs_term per-point scalars + cs_to_affine, 2 launches)", "each  (scale_each, 1 launch)"};
  double med[2];
  for (int w = 0; w < 2; ++w) {
    std::sort(t[w].begin(), t[w].end());
    med[w] = t[w][t[w].size() / 2];
    printf("G%d %-62s 2^%d points: median %9.3f ms (min %9.3f, max %9.3f, %d rounds) = %7.1f ns per point\n", group, name[w],
           log2n, med[w], t[w].front(), t[w].back(), rounds, med[w] * 1e6 / (double)n);
  }
  printf("G%d plain / each = %.3f; outputs identical\n", group, med[0] / med[1]);
  CHECK(hipFree(d_pts));
  CHECK(hipFree(d_out[0]));
  CHECK(hipFree(d_out[1]));
  CHECK(hipFree(d_work));
  CHECK(hipFree(d_k));
  return 0;
}

int main(int argc, char** argv) {
  const int group = argc > 1 ? atoi(argv[1]) : 1, log2n = argc > 2 ? atoi(argv[2]) : 20,
            rounds = argc > 3 ? atoi(argv[3]) : 7;
  if ((group != 1 && group != 2) || log2n < 0 || log2n > 24 || rounds < 1) {
    fprintf(stderr, "usage: ubench_scale_each [group 1|2] [log2n <= 24] [rounds]\n");
    return 1;
  }
  g16_ctx* ctx = nullptr;
  if (g16_ctx_create(0, &ctx) != G16_OK) {
    fprintf(stderr, "no usable GPU\n");
    return 1;
  }
  const int rc = group == 1 ? bench<G1>(ctx, 1, log2n, rounds) : bench<G2>(ctx, 2, log2n, rounds);
  g16_ctx_destroy(ctx);
  return rc;
}
