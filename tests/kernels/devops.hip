// Test-only: the op table of devops.inc as gfx950 kernels -- one kernel per op, 64-thread blocks, one operand tuple per
// lane.  Compiled once per arithmetic configuration of the product (nim_groth16_amd/csrc/Makefile takes the flags from
// the variables the product objects use) into libg16devops.so; tests/test_gpu_device_ops.py loads it through ctypes.
//   -DDEVOPS_VARIANT=<name> -DDEVOPS_VARIANT_ID=<0..4>: plain, g1acc, serial, g2acc, calls
#if !defined(DEVOPS_VARIANT) || !defined(DEVOPS_VARIANT_ID)
#error "devops.hip: build through nim_groth16_amd/csrc/Makefile (DEVOPS_VARIANT, DEVOPS_VARIANT_ID)"
#endif
// each variant must be compiled with the macros of the product configuration it stands for, and no others
#if DEVOPS_VARIANT_ID == 0   // plain: the reduce / misc kernels
#if defined(G16_F29_ASM) || defined(G16_F29_SERIAL) || defined(G16_F29_PAIR) || defined(G16_F29_PAIR_ASM) || defined(G16_FP2_CALLS)
#error "devops variant plain: no arithmetic configuration macro may be defined"
#endif
#elif DEVOPS_VARIANT_ID == 1   // g1acc: G1_ACCUM_FLAGS
#if !defined(G16_F29_ASM)
#error "devops variant g1acc: expected G16_F29_ASM from G1_ACCUM_FLAGS"
#endif
#elif DEVOPS_VARIANT_ID == 2   // serial: the pinned C++ chains
#if !defined(G16_F29_SERIAL) || defined(G16_F29_PAIR) || defined(G16_F29_ASM)
#error "devops variant serial: expected G16_F29_SERIAL alone"
#endif
#elif DEVOPS_VARIANT_ID == 3   // g2acc: G2_ACCUM_FLAGS
#if !defined(G16_F29_SERIAL) || !defined(G16_F29_PAIR) || !defined(G16_F29_PAIR_ASM)
#error "devops variant g2acc: expected G16_F29_SERIAL, G16_F29_PAIR and G16_F29_PAIR_ASM from G2_ACCUM_FLAGS"
#endif
#elif DEVOPS_VARIANT_ID == 4   // calls: Fp2 products as device function calls (make DEV=1)
#if !defined(G16_FP2_CALLS) || defined(G16_F29_ASM) || defined(G16_F29_SERIAL) || defined(G16_F29_PAIR)
#error "devops variant calls: expected G16_FP2_CALLS alone"
#endif
#else
#error "devops.hip: unknown DEVOPS_VARIANT_ID"
#endif

#include "../../nim_groth16_amd/csrc/msm.cuh"
#include "../../nim_groth16_amd/csrc/pairing.cuh"
#define DEVOPS_WITH_MSM 1
// pairing.o ships as plain, and as calls under DEV=1; the reduced-radix macros of the other builds do not reach
// pairing.cuh, so those builds leave the pairing ops out (devops_carries says so; running one there is an error)
#define DEVOPS_PAIRING (DEVOPS_VARIANT_ID == 0 || DEVOPS_VARIANT_ID == 4)
#include "devops.inc"

namespace {   // internal linkage: five variants of these templates live in one shared library

template <int OP>
__global__ void __launch_bounds__(64) devops_kernel(const uint32_t* __restrict__ in, size_t n, uint32_t* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  devops::Op<OP>::run(in + i * devops::Op<OP>::in_words, out + i * devops::Op<OP>::out_words);
}

template <int OP = 0>
hipError_t launch(int op, const uint32_t* in, size_t n, uint32_t* out) {
  if (op == OP) {
    if constexpr (devops::Op<OP>::carried) {
      devops_kernel<OP><<<dim3((unsigned)((n + 63) / 64)), dim3(64)>>>(in, n, out);
      return hipGetLastError();
    } else {
      return hipErrorInvalidValue;
    }
  }
  if constexpr (OP + 1 < devops::NOPS) return launch<OP + 1>(op, in, n, out);
  return hipErrorInvalidValue;
}

}  // namespace

#define DEVOPS_CAT2(a, b) a##b
#define DEVOPS_CAT(a, b) DEVOPS_CAT2(a, b)

// whether this variant carries the op: 1 / 0
extern "C" int DEVOPS_CAT(devops_carries_, DEVOPS_VARIANT)(int op) { return devops::carries(op) ? 1 : 0; }

// allocate, copy in, ONE launch, copy out, free.  -> the HIP error code (0 = ok), -1 = unknown op / bad argument,
// -2 = an op this variant does not carry
extern "C" int DEVOPS_CAT(devops_run_, DEVOPS_VARIANT)(int op, const void* in, size_t n, void* out) {
  const char* name;
  uint32_t inw, outw;
  if (!devops::info(op, name, inw, outw) || !in || !out || n > (size_t(1) << 24)) return -1;
  if (!devops::carries(op)) return -2;
  if (n == 0) return 0;
  const size_t inb = n * inw * 4, outb = n * outw * 4;
  uint32_t *din = nullptr, *dout = nullptr;
  hipError_t e = hipMalloc((void**)&din, inb);
  if (e == hipSuccess) e = hipMalloc((void**)&dout, outb);
  if (e == hipSuccess) e = hipMemcpy(din, in, inb, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemset(dout, 0, outb);
  if (e == hipSuccess) e = launch<0>(op, din, n, dout);
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(out, dout, outb, hipMemcpyDeviceToHost);
  if (din) (void)hipFree(din);
  if (dout) (void)hipFree(dout);
  return (int)e;
}

#if DEVOPS_VARIANT_ID == 0
extern "C" {
int devops_run_g1acc(int, const void*, size_t, void*);
int devops_run_serial(int, const void*, size_t, void*);
int devops_run_g2acc(int, const void*, size_t, void*);
int devops_run_calls(int, const void*, size_t, void*);
int devops_carries_g1acc(int);
int devops_carries_serial(int);
int devops_carries_g2acc(int);
int devops_carries_calls(int);
int devops_nops() { return devops::NOPS; }
int devops_nvariants() { return 5; }
const char* devops_variant_name(int v) {
  static const char* const names[5] = {"plain", "g1acc", "serial", "g2acc", "calls"};
  return v >= 0 && v < 5 ? names[v] : nullptr;
}
// op -> name, words per tuple in and out.  -> 0, or -1 for an unknown op
int devops_info(int op, const char** name, uint32_t* in_words, uint32_t* out_words) {
  return devops::info(op, *name, *in_words, *out_words) ? 0 : -1;
}
// 1 / 0, or -1 for an unknown variant
int devops_carries(int variant, int op) {
  switch (variant) {
    case 0: return devops_carries_plain(op);
    case 1: return devops_carries_g1acc(op);
    case 2: return devops_carries_serial(op);
    case 3: return devops_carries_g2acc(op);
    case 4: return devops_carries_calls(op);
    default: return -1;
  }
}
int devops_run(int variant, int op, const void* in, size_t n, void* out) {
  switch (variant) {
    case 0: return devops_run_plain(op, in, n, out);
    case 1: return devops_run_g1acc(op, in, n, out);
    case 2: return devops_run_serial(op, in, n, out);
    case 3: return devops_run_g2acc(op, in, n, out);
    case 4: return devops_run_calls(op, in, n, out);
    default: return -1;
  }
}
}
#endif
