// Instantiates the pooled tile kernels (score_pool_kernels.h) for one model; one translation unit per model so the
// five families compile in parallel.
#include "score_pool_launch.h"

namespace mkb {
template int pool_launch<MKB_TRANSE, true>(int, const PoolPlan &, const PoolArgs &, hipStream_t);
template int pool_launch<MKB_TRANSE, false>(int, const PoolPlan &, const PoolArgs &, hipStream_t);
}  // namespace mkb
