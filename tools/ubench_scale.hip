// Micro-benchmark of one scalar times an array of G1 points, two ways in one process on the same points and scalar:
//   plain    the arithmetic the circuit setup used for its delta^-1 scaling before scale.cuh existed: cs_term<G1> with one
//            scalar for all (the 254-bit ladder of scalar_mul.cuh per lane, XYZZ written to global memory) and then
//            cs_to_affine<G1> (one field inversion per point), two launches, the very kernels of circuit_setup.cuh;
//   uniform  scale_uniform<G1> (scale.cuh): the uploaded joint-sparse-form schedule over the endomorphism, one inversion
//            per four points, one launch.
//
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 -Iinclude tools/ubench_scale.hip -Lnim_groth16_amd/csrc -lg16hip
//         -Wl,-rpath,$PWD/nim_groth16_amd/csrc -o tools/ubench_scale
//   tools/ubench_scale [log2n = 20] [rounds = 7]
//
// The points are multiples of gen1 by random scalars (g16_fixed_base_g1), the scalar is one more random draw.  The two
// paths alternate after one warm-up each; times are HIP events around the launches of a path; the outputs must agree
// byte for byte.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../include/g16hip.h"
#include "../nim_groth16_amd/csrc/circuit_setup.cuh"
#include "../nim_groth16_amd/csrc/scale.cuh"

using namespace g16;

#define CHECK(x)                                                                      \
  do {                                                                                \
    hipError_t e__ = (x);                                                             \
    if (e__ != hipSuccess) {                                                          \
      fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e__));                        \
      exit(1);                                                                        \
    }                                                                                 \
  } while (0)

int main(int argc, char** argv) {
  const int log2n = argc > 1 ? atoi(argv[1]) : 20, rounds = argc > 2 ? atoi(argv[2]) : 7;
  if (log2n < 0 || log2n > 24 || rounds < 1) {
    fprintf(stderr, "usage: ubench_scale [log2n <= 24] [rounds]\n");
    return 1;
  }
  const size_t n = size_t(1) << log2n;
  g16_ctx* ctx = nullptr;
  if (g16_ctx_create(0, &ctx) != G16_OK) {
    fprintf(stderr, "no usable GPU\n");
    return 1;
  }
  // random scalars below 2^253 (SplitMix64), standard form; the last one is k
  std::vector<uint64_t> sc(4 * (n + 1));
  uint64_t state = 20;
  for (auto& w : sc) {
    uint64_t z = (state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    w = z ^ (z >> 31);
  }
  for (size_t i = 0; i <= n; ++i) sc[4 * i + 3] &= 0x1fffffffffffffffull;
  std::vector<g1_aff> pts(n);
  if (g16_fixed_base_g1(ctx, sc.data(), G16_SCALARS_STD, n, pts.data()) != G16_OK) {
    fprintf(stderr, "g16_fixed_base_g1: %s\n", g16_last_error(ctx));
    return 1;
  }
  U256 k;
  memcpy(k.v, &sc[4 * n], 32);
  bool ok = false;
  const ScalePlan plan = make_scale_plan(k, &ok);
  if (!ok || !scale_plan_is(plan, k)) {
    fprintf(stderr, "the plan of k does not evaluate to k\n");
    return 1;
  }
  ScaleArgs args;
  memcpy(args.k.v, k.v, 32);
  args.nsteps = (uint32_t)plan.nsteps, args.tail_dbls = (uint32_t)plan.tail_dbls;

  g1_aff *d_pts, *d_out[2];
  g1_acc* d_work;
  u256* d_k;
  uint32_t* d_steps;
  CHECK(hipMalloc(&d_pts, n * sizeof(g1_aff)));
  CHECK(hipMalloc(&d_out[0], n * sizeof(g1_aff)));
  CHECK(hipMalloc(&d_out[1], n * sizeof(g1_aff)));
  CHECK(hipMalloc(&d_work, n * sizeof(g1_acc)));
  CHECK(hipMalloc(&d_k, 32));
  CHECK(hipMalloc(&d_steps, ScalePlan::MAX_STEPS * 4));
  CHECK(hipMemcpy(d_pts, pts.data(), n * sizeof(g1_aff), hipMemcpyHostToDevice));
  CHECK(hipMemcpy(d_k, k.v, 32, hipMemcpyHostToDevice));
  CHECK(hipMemcpy(d_steps, plan.step, sizeof(ScaleStep) * (size_t)plan.nsteps, hipMemcpyHostToDevice));
  args.steps = d_steps;
  hipEvent_t e0, e1;
  CHECK(hipEventCreate(&e0));
  CHECK(hipEventCreate(&e1));
  auto run = [&](int which) {
    CHECK(hipEventRecord(e0));
    if (which == 0) {
      hipLaunchKernelGGL(cs_term<G1>, dim3(cs_grid(n)), dim3(CS_BLOCK), 0, 0, (const g1_aff*)d_pts,
                         (const uint32_t*)nullptr, (const u256*)d_k, (const uint32_t*)nullptr, 0u, 0u, 0u, (uint32_t)n,
                         d_work);
      hipLaunchKernelGGL(cs_to_affine<G1>, dim3(cs_grid(n)), dim3(CS_BLOCK), 0, 0, (const g1_acc*)d_work, (uint32_t)n,
                         d_out[0]);
    } else {
      hipLaunchKernelGGL(scale_uniform<G1>, dim3((uint32_t)((n + SCALE_TILE - 1) / SCALE_TILE)), dim3(SCALE_BLOCK), 0, 0,
                         (const g1_aff*)d_pts, (uint32_t)n, args, d_out[1]);
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
  std::vector<g1_aff> got[2] = {std::vector<g1_aff>(n), std::vector<g1_aff>(n)};
  for (int w = 0; w < 2; ++w) CHECK(hipMemcpy(got[w].data(), d_out[w], n * sizeof(g1_aff), hipMemcpyDeviceToHost));
  if (memcmp(got[0].data(), got[1].data(), n * sizeof(g1_aff))) {
    fprintf(stderr, "the two paths differ\n");
    return 1;
  }
  const char* name[2] = {"plain   (cs_term<G1> one scalar + cs_to_affine<G1>, 2 launches)",
                         "uniform (scale_uniform<G1>, 1 launch)"};
  double med[2];
  printf("k: %d steps, %d doublings (254-bit ladder: 254 doublings)\n", plan.nsteps, plan.ndbl);
  for (int w = 0; w < 2; ++w) {
    std::sort(t[w].begin(), t[w].end());
    med[w] = t[w][t[w].size() / 2];
    printf("%-66s 2^%d points: median %9.3f ms (min %9.3f, max %9.3f, %d rounds) = %7.1f ns per point\n", name[w], log2n,
           med[w], t[w].front(), t[w].back(), rounds, med[w] * 1e6 / (double)n);
  }
  printf("uniform / plain = %.3f; outputs identical\n", med[1] / med[0]);
  CHECK(hipFree(d_pts));
  CHECK(hipFree(d_out[0]));
  CHECK(hipFree(d_out[1]));
  CHECK(hipFree(d_work));
  CHECK(hipFree(d_k));
  CHECK(hipFree(d_steps));
  g16_ctx_destroy(ctx);
  return 0;
}
