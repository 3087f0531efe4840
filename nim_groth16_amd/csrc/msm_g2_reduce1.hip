// G2 split-bucket combine and first bucket-reduction stage
#include "msm_stage.cuh"
template int32_t stage_heavy<G2>(g16_ctx*, hipStream_t, const MsmParams&, const MsmTailPlan&, const MsmBatch<G2>&, uint32_t);
template int32_t stage_reduce1<G2>(g16_ctx*, hipStream_t, const MsmParams&, const MsmTailPlan&, const MsmBatch<G2>&, uint32_t);
