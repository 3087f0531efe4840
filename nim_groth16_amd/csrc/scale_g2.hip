// The G2 kernel of the uniform scaling (scale.cuh): the bit ladder with the grouped affine conversion.
#include "scale.cuh"

namespace g16 {
template int32_t scale_uniform_device<G2>(g16_ctx*, const void*, size_t, const ScaleJob&, void*);
}  // namespace g16
