// The G2 kernels of the circuit setup (circuit_setup.cuh): LG2 and pointsB2.
#include "circuit_setup.cuh"

namespace g16 {
CS_INSTANTIATE(G2)
}  // namespace g16
