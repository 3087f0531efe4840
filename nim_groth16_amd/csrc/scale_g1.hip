// The G1 kernel of the uniform scaling (scale.cuh): the endomorphism ladder over the uploaded schedule.
#include "scale.cuh"

namespace g16 {
template int32_t scale_uniform_device<G1>(g16_ctx*, const void*, size_t, const ScaleJob&, void*);
}  // namespace g16
