// G2 bucket-segment accumulation (the dominant kernel of the MSM)
#include "msm_stage.cuh"
template int32_t stage_accum<G2>(g16_ctx*, hipStream_t, const MsmParams&, const MsmBatch<G2>&, uint32_t);
