// Pass plans of the NTT (ntt.hip), shared by host code and by the CPU test shim: the three workgroup geometries
// (ntt.cuh), how a 2^log2n transform is split into passes, and the LDS each pass asks for.  Plain C++: the shim is
// built with g++.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace g16 {

// G16_NTT_TILE = 1024 | 2048 | 4096 (ntt.cuh): a tile of 2^log2tile elements, passes of at most max_rho stages
struct NttGeom {
  uint32_t log2tile, max_rho;
};
constexpr NttGeom ntt_geom(int tile) {
  return tile == 1024 ? NttGeom{10, 8} : tile == 4096 ? NttGeom{12, 10} : NttGeom{11, 10};
}

// dynamic LDS of a pass: tile + R/2 inner twiddles.  Up to 144 KB: above the 64 KB default, so the kernels are
// opted in once per process, to ntt_optin_shmem().
constexpr size_t ntt_pass_shmem(uint32_t rho, uint32_t log2b) {
  return (size_t(32) << (rho + log2b)) + (size_t(16) << rho);
}
constexpr size_t ntt_optin_shmem() { return ntt_pass_shmem(10, 2); }

// a transform of 2^log2n <= 2^max_rho is ONE pass (which cannot run in place)
constexpr bool ntt_one_pass(NttGeom g, uint32_t log2n) { return log2n <= g.max_rho; }

// passes of <= max_rho stages: one up to 2^max_rho, two up to 2^(2 max_rho), three beyond (four for the 1024 geometry
// beyond 2^24).  log2n == 0 is one pass of no stage (only the fused quotient pass launches it).
constexpr uint32_t ntt_npass(NttGeom g, uint32_t log2n) { return log2n ? (log2n + g.max_rho - 1) / g.max_rho : 1; }

// pass p: rho stages (the first log2n % npass passes take one more) over tiles of 2^log2b bases, after log2s stages
struct NttPass {
  uint32_t rho, log2b, log2s, ntiles;
  size_t shmem;
};
constexpr NttPass ntt_pass_plan(NttGeom g, uint32_t log2n, uint32_t p) {
  const uint32_t npass = ntt_npass(g, log2n);
  uint32_t log2s = 0;
  for (uint32_t q = 0; q < p; ++q) log2s += log2n / npass + (q < log2n % npass ? 1u : 0u);
  const uint32_t rho = log2n / npass + (p < log2n % npass ? 1u : 0u);
  uint32_t log2b = g.log2tile - rho;
  if (log2b > log2n - rho) log2b = log2n - rho;
  return NttPass{rho, log2b, log2s, 1u << (log2n - rho - log2b), ntt_pass_shmem(rho, log2b)};
}

}  // namespace g16
