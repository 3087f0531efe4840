// Test-only: the op table of tests/kernels/devops.inc compiled with g++, i.e. through the portable (#else) branches of
// the device headers: the same operand vectors as the GPU test, on a machine without a GPU.  A library of its own
// (not part of ffec_shim.cpp): inlining every op takes g++ minutes.
#include <stddef.h>

#include "../../nim_groth16_amd/csrc/ec29.cuh"
#include "../../nim_groth16_amd/csrc/pairing.cuh"
#include "../kernels/devops.inc"

template <int OP = 0>
static int host_run(int op, const uint32_t* in, size_t n, uint32_t* out) {
  if (op == OP) {
    for (size_t i = 0; i < n; ++i) devops::Op<OP>::run(in + i * devops::Op<OP>::in_words, out + i * devops::Op<OP>::out_words);
    return 0;
  }
  if constexpr (OP + 1 < devops::NOPS) return host_run<OP + 1>(op, in, n, out);
  return -1;
}

extern "C" {
int devops_nops() { return devops::NOPS; }
// op -> name, words per tuple in and out.  -> 0, or -1 for an unknown op
int devops_info(int op, const char** name, uint32_t* in_words, uint32_t* out_words) {
  return devops::info(op, *name, *in_words, *out_words) ? 0 : -1;
}
// one tuple after the other.  -> 0, or -1 for an unknown op
int devops_host_run(int op, const void* in, size_t n, void* out) {
  return host_run<0>(op, (const uint32_t*)in, n, (uint32_t*)out);
}
}
