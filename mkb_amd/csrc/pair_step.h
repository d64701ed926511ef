// The pooled backward's pair step: given a lane's KPT units of a query row q and of a candidate row x and the seed
// g = d loss / d score of the pair, add the pair's gradient into dq and / or dx.  Written once for the kernels of
// score_pool_kernels.h, on top of the per-unit formulas of model_math.h.
//
// Arrays are a lane's KPT consecutive units: a0 = re / real parts, a1 = im parts (RotatE only; zeros otherwise).
// The forms round differently (separate multiply and add, fused multiply-add, one or two rows per packed chain), so a
// kernel keeps the form it was written and measured with; they are not interchangeable bit for bit.
// A caller that wants one of the two gradients passes a local it never reads for the other: the helpers are inlined,
// and the compiler drops the products nobody reads.
#pragma once
#include "model_math.h"

namespace mkb {

// One row, both gradients, unit by unit: pair_bwd_cmod (RotatE) or pair_bwd_real.  extra accumulates g * |sin z|,
// pRotatE's modulus gradient.
template <int MODEL, bool HEAD, int KPT>
__device__ __forceinline__ void pair_step(const float (&q0)[KPT], const float (&q1)[KPT], const float (&x0)[KPT],
                                          const float (&x1)[KPT], float g, float kd, float modulus, float (&dq0)[KPT],
                                          float (&dq1)[KPT], float (&dx0)[KPT], float (&dx1)[KPT], float &extra) {
#pragma unroll
    for (int v = 0; v < KPT; ++v) {
        if constexpr (ModelTraits<MODEL>::cplx_pair) {
            Cplx dq, dx;
            pair_bwd_cmod(Cplx{q0[v], q1[v]}, Cplx{x0[v], x1[v]}, g, dq, dx);
            dq0[v] += dq.re; dq1[v] += dq.im;
            dx0[v] += dx.re; dx1[v] += dx.im;
        } else {
            float dq, dx, e0 = 0.f;
            pair_bwd_real<MODEL, HEAD>(q0[v], x0[v], g, kd, modulus, dq, dx, e0);
            dq0[v] += dq;
            dx0[v] += dx;
            extra += g * e0;
        }
    }
}

// One row, ONE gradient, unit by unit: the scalar form of the two-pass kernels.  acc is dq (DX = false) or the candidate's
// gradient (DX = true); the other one goes to a local nobody reads.  extra is pRotatE's; only the dq pass reads it afterwards.
template <int MODEL, bool HEAD, int KPT, bool DX>
__device__ __forceinline__ void pair_step_one(const float (&q0)[KPT], const float (&q1)[KPT], const float (&x0)[KPT],
                                              const float (&x1)[KPT], float g, float kd, float modulus,
                                              float (&acc0)[KPT], float (&acc1)[KPT], float &extra) {
    float n0[KPT], n1[KPT];
#pragma unroll
    for (int v = 0; v < KPT; ++v) { n0[v] = 0.f; n1[v] = 0.f; }
    if constexpr (DX) pair_step<MODEL, HEAD, KPT>(q0, q1, x0, x1, g, kd, modulus, n0, n1, acc0, acc1, extra);
    else pair_step<MODEL, HEAD, KPT>(q0, q1, x0, x1, g, kd, modulus, acc0, acc1, n0, n1, extra);
}

}  // namespace mkb
