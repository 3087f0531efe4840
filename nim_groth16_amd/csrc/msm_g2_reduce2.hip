// G2 second bucket-reduction stage, fold, and the sum of per-GPU partials
#include "msm_stage.cuh"
template int32_t stage_reduce2_fold<G2>(g16_ctx*, hipStream_t, const MsmParams&, const MsmTailPlan&, const MsmBatch<G2>&, uint32_t);
template int32_t sum_partials_device<G2>(g16_ctx*, const void*, uint32_t, void*);
