// The G1 kernel of the per-point scaling (scale_each.cuh): the endomorphism ladder over the lane's own split scalar.
#include "scale_each.cuh"

namespace g16 {
template int32_t scale_each_device<G1>(g16_ctx*, const void*, size_t, const void*, uint32_t, void*);
}  // namespace g16
