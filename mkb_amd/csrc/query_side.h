// The query side of a score, written once: every score is pair(q_i, x) (model_math.h), q_i is built from the two fixed
// operands of sample row i (h and r; r and t for head-batch) and its gradient is chained back into those operands' rows.
// What a kernel needs to know about that lives here: where the row's operands are, how a unit of them is laid out, how a
// unit of q is built and how dq goes back.  The general kernels (score_general.hip, score_relation.hip, score_cand.hip), the
// pooled path's row kernels (score_pool.hip) and the all-entity evaluation (rank.hip) all go through it.
//
// Units: real models have one float per unit (De units per row).  Complex-query models (RotatE, ComplEx) have d complex
// units per row, re at u and im at d + u; ComplEx's relation row has an imaginary half as well, RotatE's holds d phases.
#pragma once
#include "model_math.h"

namespace mkb {

// Row i of `sample`: its ids, the three operand rows and what the loops over its units need.
struct QueryRow {
    int64_t h, r, t;
    const float *eh, *er, *et;
    int d, U;  // U: units per row (d for complex-query models, De otherwise)
    float kd;
    template <bool HEAD> __device__ __forceinline__ const float *ent() const { return HEAD ? et : eh; }  // the query's entity operand
    template <bool HEAD> __device__ __forceinline__ int64_t ent_id() const { return HEAD ? t : h; }
};

// A: anything with the table fields ent, rel, De, Dr, d, kd (TablesDev, RowArgs, RowStepArgs)
template <int MODEL, class Args>
__device__ __forceinline__ QueryRow query_row(const Args &A, const int64_t *__restrict__ sample, int64_t i) {
    QueryRow R;
    R.h = sample[3 * i]; R.r = sample[3 * i + 1]; R.t = sample[3 * i + 2];
    R.eh = A.ent + R.h * A.De; R.er = A.rel + R.r * A.Dr; R.et = A.ent + R.t * A.De;
    R.d = A.d;
    R.U = ModelTraits<MODEL>::cplx_query ? A.d : (int)A.De;
    R.kd = A.kd;
    return R;
}

// ---------------------------------------------------------------- operand loads (complex-query models; real ones read row[u])
__device__ __forceinline__ Cplx ent_unit(const float *e, int d, int u) { return Cplx{e[u], e[d + u]}; }
template <int MODEL>
__device__ __forceinline__ Cplx rel_unit(const float *er, int d, int u) { return Cplx{er[u], MODEL == MKB_COMPLEX ? er[d + u] : 0.f}; }
// ... and for any model: the halves the row has (a real model's unit is its .re); rel_unit<MODEL> already is that
template <int MODEL>
__device__ __forceinline__ Cplx ent_unit(const float *e, int d, int u) {
    return Cplx{e[u], ModelTraits<MODEL>::cplx_query ? e[d + u] : 0.f};
}

// ---------------------------------------------------------------- one unit of q and of its chain, on loaded operands
// e = the entity operand (h; t for head-batch), r = the relation operand, whichever side the query is built for
template <int MODEL, bool HEAD>
__device__ __forceinline__ float query_of(float e, float r, float kd) {
    return HEAD ? build_q_real<MODEL, true>(r, e, kd) : build_q_real<MODEL, false>(e, r, kd);
}
template <int MODEL, bool HEAD>
__device__ __forceinline__ Cplx query_of(Cplx e, Cplx r, float kd) { return build_q_cplx<MODEL, HEAD>(e, r, kd); }

// dq -> (de, dr): the contributions to the entity operand's and the relation operand's gradient
template <int MODEL, bool HEAD>
__device__ __forceinline__ void query_chain(float e, float r, float dq, float kd, float &de, float &dr) {
    if constexpr (HEAD) query_bwd_real<MODEL, true>(r, e, dq, kd, dr, de);
    else query_bwd_real<MODEL, false>(e, r, dq, kd, de, dr);
}
template <int MODEL, bool HEAD>
__device__ __forceinline__ void query_chain(Cplx e, Cplx r, Cplx dq, float kd, Cplx &de, Cplx &dr) {
    query_bwd_cplx<MODEL, HEAD>(e, r, dq, kd, de, dr);
}

// ---------------------------------------------------------------- the same for unit u of a row
// Real models: q0 (q1 = 0).  Complex-query models: (q0, q1) = (re, im).
template <int MODEL, bool HEAD>
__device__ __forceinline__ void query_unit(const QueryRow &R, int u, float &q0, float &q1) {
    if constexpr (ModelTraits<MODEL>::cplx_query) {
        const Cplx q = query_of<MODEL, HEAD>(ent_unit(R.ent<HEAD>(), R.d, u), rel_unit<MODEL>(R.er, R.d, u), R.kd);
        q0 = q.re; q1 = q.im;
    } else {
        float e, r;  // loaded in build_q_real's operand order (the compiler's schedule follows it)
        if constexpr (HEAD) { r = R.er[u]; e = R.et[u]; } else { e = R.eh[u]; r = R.er[u]; }
        q0 = query_of<MODEL, HEAD>(e, r, R.kd);
        q1 = 0.f;
    }
}

// Returns the contributions; how they are added is the caller's business (real models: the .re halves only).  dq comes by
// reference so that it is read after the operands are loaded: the compiler orders the products' factors by that.
template <int MODEL, bool HEAD>
__device__ __forceinline__ void query_unit_bwd(const QueryRow &R, int u, const float &dq0, const float &dq1, Cplx &de, Cplx &dr) {
    if constexpr (ModelTraits<MODEL>::cplx_query) {
        query_chain<MODEL, HEAD>(ent_unit(R.ent<HEAD>(), R.d, u), rel_unit<MODEL>(R.er, R.d, u), Cplx{dq0, dq1}, R.kd, de, dr);
    } else {
        float e, r;  // (as in query_unit)
        if constexpr (HEAD) { r = R.er[u]; e = R.et[u]; } else { e = R.eh[u]; r = R.er[u]; }
        query_chain<MODEL, HEAD>(e, r, dq0, R.kd, de.re, dr.re);
        de.im = dr.im = 0.f;
    }
}

// ... and the common way to add them: one atomic per element into a gradient row (duplicate rows add).  Which halves the row
// has: an entity row both for the complex-query models, a relation row only ComplEx's.
template <int MODEL, bool REL_ROW>
__device__ __forceinline__ void row_grad_atomic(float *g_row, int d, int u, Cplx v) {
    atomicAdd(g_row + u, v.re);
    if constexpr (ModelTraits<MODEL>::cplx_query && (!REL_ROW || MODEL == MKB_COMPLEX)) atomicAdd(g_row + d + u, v.im);
}
// Both operands' rows, issued in operand order, like the loads: a head-batch real model's relation comes first.
template <int MODEL, bool HEAD>
__device__ __forceinline__ void query_grad_atomic(float *g_e, float *g_r, int d, int u, Cplx de, Cplx dr) {
    constexpr bool rel_first = HEAD && !ModelTraits<MODEL>::cplx_query;
    if constexpr (rel_first) row_grad_atomic<MODEL, true>(g_r, d, u, dr);
    row_grad_atomic<MODEL, false>(g_e, d, u, de);
    if constexpr (!rel_first) row_grad_atomic<MODEL, true>(g_r, d, u, dr);
}

// ---------------------------------------------------------------- Q[i] = query of row i, one workgroup of 256 lanes per row
struct RowArgs {
    const float *ent, *rel;
    const int64_t *sample;
    float *Q;          // [B, De] out (build) / [nslices, B, De] dQ partials in (backward)
    float *g_ent, *g_rel;
    int64_t De, Dr;
    int d, B, nslices;
    float kd;
    // GEMM route: depth[i] = one past the last pool position row i uses (cnt [B, P]); null = not wanted
    const uint16_t *cnt;
    int *depth;
    int P;
};

// RowArgs of a query build alone (the general path, the evaluation): no gradient rows, no dQ slices, no depth scan
inline RowArgs query_build_args(const float *ent, const float *rel, const int64_t *sample, float *Q, int64_t De, int64_t Dr, int d,
                                int64_t B, float kd) {
    RowArgs A{};
    A.ent = ent; A.rel = rel; A.sample = sample; A.Q = Q;
    A.De = De; A.Dr = Dr; A.d = d; A.B = (int)B; A.nslices = 1; A.kd = kd;
    A.depth = nullptr;  // query_build_kernel skips the scan
    return A;
}

// depth[i] for the GEMM route's "used pool depth" cuts (gemm_mfma.h): one workgroup per row scans the row's multiplicities
__device__ __forceinline__ void row_depth_256(const uint16_t *__restrict__ cnt, int P, int64_t i, int *__restrict__ depth) {
    __shared__ int s_dep[4];
    int m = 0;
    for (int p = threadIdx.x; p < P; p += 256)
        if (cnt[i * P + p]) m = p + 1;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m = max(m, __shfl_xor(m, off, 64));
    if ((threadIdx.x & 63) == 0) s_dep[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) depth[i] = max(max(s_dep[0], s_dep[1]), max(s_dep[2], s_dep[3]));
}

template <int MODEL, bool HEAD>
__global__ __launch_bounds__(256) void query_build_kernel(RowArgs A) {
    const int64_t i = blockIdx.x;
    if (A.depth) row_depth_256(A.cnt, A.P, i, A.depth);
    const QueryRow R = query_row<MODEL>(A, A.sample, i);
    float *q = A.Q + i * A.De;
    for (int u = threadIdx.x; u < R.U; u += 256) {
        float q0, q1;
        query_unit<MODEL, HEAD>(R, u, q0, q1);
        q[u] = q0;
        if constexpr (ModelTraits<MODEL>::cplx_query) q[R.d + u] = q1;
    }
}

}  // namespace mkb
