// CPU build of the scalar side of the fake setup (nim_groth16_amd/csrc/setup.cuh) for tests/test_setup_cpu.py: the
// per-run function of the geometric / Lagrange kernel, the combination of one wire, and the small host helpers, with the
// exact code the device runs.
#include "../../nim_groth16_amd/csrc/setup.cuh"
#include <cstdint>
#include <cstring>

using namespace g16;

extern "C" {

int shim_run_length() { return SETUP_RUN; }
int shim_block_size() { return SETUP_BLOCK; }

uint32_t shim_log2_domain(uint32_t nconstraints, uint32_t npubs) { return setup_log2_domain(nconstraints, npubs); }

// Montgomery Fr in and out (32 bytes each)
void shim_omega(uint32_t log2n, void* out) {
  const u256 w = setup_omega(log2n);
  memcpy(out, &w, 32);
}
void shim_pow(const void* b, uint32_t e, void* out) {
  u256 x;
  memcpy(&x, b, 32);
  x = setup_pow_u32(x, e);
  memcpy(out, &x, 32);
}

// one run of `len` <= SETUP_RUN elements from x0; out: SETUP_RUN + 1 slots of 32 bytes that the caller has filled with
// a pattern (slots at and beyond len must come back untouched).  Returns the position of the first zero denominator or
// SETUP_RUN.
uint32_t shim_geom_run(int lagrange, const void* x0, const void* s, const void* c, const void* tau, uint32_t len, void* out) {
  u256 a[4];
  memcpy(&a[0], x0, 32), memcpy(&a[1], s, 32), memcpy(&a[2], c, 32), memcpy(&a[3], tau, 32);
  u256 o[SETUP_RUN + 1];
  memcpy(o, out, sizeof o);
  const uint32_t z = lagrange ? setup_geom_run<SETUP_RUN, true>(a[0], a[1], a[2], a[3], len, o)
                              : setup_geom_run<SETUP_RUN, false>(a[0], a[1], a[2], a[3], len, o);
  memcpy(out, o, sizeof o);
  return z;
}

// in: a, b, c, alpha, beta, gamma^-1, delta^-1 (7 x 32 bytes)
void shim_combine(const void* in, uint32_t j, uint32_t npubs, void* out) {
  u256 v[7];
  memcpy(v, in, sizeof v);
  const u256 r = setup_combine(v[0], v[1], v[2], v[3], v[4], v[5], v[6], j, npubs);
  memcpy(out, &r, 32);
}

}  // extern "C"
