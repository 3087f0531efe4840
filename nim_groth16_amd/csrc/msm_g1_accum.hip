// G1 bucket-segment accumulation (the dominant kernel of the MSM)
#include "msm_stage.cuh"
template int32_t stage_accum<G1>(g16_ctx*, hipStream_t, const MsmParams&, const MsmBatch<G1>&, uint32_t);
