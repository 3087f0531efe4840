// The G1 kernels of the circuit setup (circuit_setup.cuh), and the point difference of the H points, which only G1 has.
#include "circuit_setup.cuh"

namespace g16 {
CS_INSTANTIATE(G1)
template int32_t cs_diff_device<G1>(g16_ctx*, const void*, const void*, size_t, void*);
}  // namespace g16
