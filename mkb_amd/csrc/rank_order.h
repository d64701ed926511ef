// The order of the filtered rank and of every top-k selection, written once (rank.hip, score_relation.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mkb {

// Position of the target in the reference's torch.argsort(score, descending=True) (evaluation.py:245-262).  Ties and NaN
// need care: "1 + #{S[e] > S[target]}" alone ranks the target FIRST whenever nothing compares greater, i.e. for a collapsed
// model (all scores equal) or a diverged one (NaN anywhere in the comparison) -- MRR = HITS@k = 1.0 for a broken run, which
// the early-stopping logic of Pipeline.learn would then keep.  The order used here is the one of a stable descending sort
// with torch's NaN convention: NaN sorts before every number, equal keys keep candidate order (lower entity id first).
__device__ __forceinline__ bool ranks_before(float a, int64_t ia, float b, int64_t ib) {
    const bool an = a != a, bn = b != b;
    if (an || bn) return an && (!bn || ia < ib);
    return a > b || (a == b && ia < ib);
}

}  // namespace mkb
