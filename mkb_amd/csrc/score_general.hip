// General (arbitrary candidate ids) scoring kernels: mkb_score_fwd / mkb_score_bwd.
//
// Replaces, for one call of model.forward(sample, negative_sample, mode) and its autograd:
//   BaseModel.batch gather (models/base.py:153-207) + <Model>.forward math (models/*.py) and the
//   index_select backward (dense index_add_), SURVEY.md a3-a8, a13.
//
// Forward  : one workgroup per batch row.  The row's query vector q_i (built from the two fixed
//            operands) is staged in LDS once and shared by all K candidates; each of the 4 waves streams
//            whole candidate rows with coalesced loads and finishes with a wave64 shuffle reduction.
// Backward : candidates given (K > 1 slots per row): two passes over the B*K pairs, lanes OWN units k in both (no cross-lane
//            reduction), neither writes a gradient per pair:
//              dq pass   one workgroup per batch row; dq accumulates in registers over the row's K candidates and is chained
//                        into the fixed operands' rows (one atomic per element and row): score_bwd_kernel<.., DX = false>;
//              dx pass   the pairs are SORTED BY CANDIDATE (pair_sort.h: a radix sort of B*K int32 keys); a workgroup walks 64
//                        consecutive sorted pairs (walk_sorted_pairs, score_row.h), keeps the candidate row and its running
//                        gradient in registers and adds them to the table gradient only when the candidate changes: B*K/64 ...
//                        #distinct flushes instead of one fp32 atomic per (pair, dim) -- 524 M at the headline shape, which
//                        was ~2/3 of the step.
//            The pair term is evaluated in both passes (cheaper than the atomics it replaces).  Positive triples
//            (no candidates, K = 1) keep the one-pass kernel: the dq pass with its per-pair gradient writes (DX = true).
//            The dx pass reads the rows' queries from Q [B, De], written by query_side.h's query_build_kernel.
// The [B,K,D] intermediates of the reference are never materialised.
#include "common.h"
#include "pair_sort.h"
#include "query_side.h"
#include "score_row.h"  // TablesDev, the pair sum of one candidate row, one pair's gradient, the walk over sorted pairs

#include <stdlib.h>

namespace mkb {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;

template <int MODEL, bool HEAD>
__global__ __launch_bounds__(kBlock) void score_fwd_kernel(TablesDev T, const int64_t *__restrict__ sample,
                                                           const int64_t *__restrict__ cand, int K,
                                                           float *__restrict__ score) {
    extern __shared__ __attribute__((aligned(16))) float q_lds[];
    const int i = blockIdx.x;
    const QueryRow R = query_row<MODEL>(T, sample, i);
    for (int u = threadIdx.x; u < R.U; u += kBlock) {
        float q0, q1;
        query_unit<MODEL, HEAD>(R, u, q0, q1);
        q_lds[u] = q0;
        if constexpr (ModelTraits<MODEL>::cplx_query) q_lds[T.d + u] = q1;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float modulus = (MODEL == MKB_PROTATE) ? T.modulus[0] : 0.f;
    const bool vec4 = T.vec4 != 0;
    for (int j = wave; j < K; j += kWaves) {
        const int64_t c = cand ? cand[(int64_t)i * K + j] : R.t;
        const float *x = T.ent + c * T.De;
        float acc = pair_row_sum<MODEL, HEAD>(T, q_lds, x, lane, vec4);
        acc = wave_sum(acc);
        if (lane == 0) score[(int64_t)i * K + j] = finish_score<MODEL>(acc, T.gamma, modulus);
    }
}

// Backward over the K candidates of a batch row: one workgroup per row, lanes own units; dq accumulates in registers and is
// chained into the fixed operands' rows (one atomic per element and row).
//   DX   the one-pass backward: also one atomic per (pair, element) into the candidate's row.  Positive triples (cand ==
//        nullptr, K = 1) score against the row's own tail.
//   !DX  the dq pass of the two-pass backward: no gradient is written per pair.
template <int MODEL, bool HEAD, bool DX>
__global__ __launch_bounds__(kBlock) void score_bwd_kernel(TablesDev T, mkb_grads_t G,
                                                           const int64_t *__restrict__ sample,
                                                           const int64_t *__restrict__ cand, int K,
                                                           const float *__restrict__ dscore) {
    __shared__ float red[kWaves];
    const int i = blockIdx.x;
    const QueryRow R = query_row<MODEL>(T, sample, i);
    float *g_e = G.g_ent + R.ent_id<HEAD>() * T.De;  // fixed entity operand of the query
    float *g_r = G.g_rel + R.r * T.Dr;
    const float modulus = (MODEL == MKB_PROTATE) ? T.modulus[0] : 0.f;
    float extra = 0.f;
    for (int u = threadIdx.x; u < R.U; u += kBlock) {
        float q0, q1;
        query_unit<MODEL, HEAD>(R, u, q0, q1);
        float dq0 = 0.f, dq1 = 0.f;
        for (int j = 0; j < K; ++j) {
            const float g = dscore[(int64_t)i * K + j];
            const int64_t c = (DX && !cand) ? R.t : cand[(int64_t)i * K + j];
            Cplx dq, dx;
            pair_unit_bwd<MODEL, HEAD>(Cplx{q0, q1}, ent_unit<MODEL>(T.ent + c * T.De, T.d, u), g, T.kd, modulus, dq, dx, extra);
            dq0 += dq.re; dq1 += dq.im;
            if constexpr (DX) row_grad_atomic<MODEL, false>(G.g_ent + c * T.De, T.d, u, dx);  // the per-pair gradient write
        }
        Cplx de, dr;
        query_unit_bwd<MODEL, HEAD>(R, u, dq0, dq1, de, dr);
        query_grad_atomic<MODEL, HEAD>(g_e, g_r, T.d, u, de, dr);
    }
    if constexpr (MODEL == MKB_PROTATE) {  // d score / d modulus = - sum_k |sin z|   (protate.py:91)
        extra = block_sum_4waves(extra, red);
        if (threadIdx.x == 0) atomicAdd(G.g_modulus, -extra);
    }
}

// dx pass of the two-pass backward: workgroup = kChunkPairs consecutive pairs of the candidate-sorted pair list
template <int MODEL, bool HEAD>
__global__ __launch_bounds__(kBlock) void score_bwd_x_kernel(TablesDev T, mkb_grads_t G, const int *__restrict__ sorted_cand,
                                                             const int *__restrict__ sorted_pair, int n_pairs, int K,
                                                             const float *__restrict__ Q, const float *__restrict__ dscore) {
    const int lo = blockIdx.x * kChunkPairs, hi = min(n_pairs, lo + kChunkPairs);
    const int U = ModelTraits<MODEL>::cplx_query ? T.d : (int)T.De;
    const float modulus = (MODEL == MKB_PROTATE) ? T.modulus[0] : 0.f;
    for (int u = threadIdx.x; u < U; u += kBlock) {
        Cplx x{0.f, 0.f}, dx{0.f, 0.f};
        float unused = 0.f;
        walk_sorted_pairs(
            sorted_cand, sorted_pair, lo, hi,
            [&](int c) {
                x = ent_unit<MODEL>(T.ent + (int64_t)c * T.De, T.d, u);
                dx = Cplx{0.f, 0.f};
            },
            [&](int pair) {
                const float g = dscore[pair];
                Cplx dq, d;
                pair_unit_bwd<MODEL, HEAD>(ent_unit<MODEL>(Q + (int64_t)(pair / K) * T.De, T.d, u), x, g, T.kd, modulus, dq, d, unused);
                dx.re += d.re; dx.im += d.im;
            },
            [&](int c) { row_grad_atomic<MODEL, false>(G.g_ent + (int64_t)c * T.De, T.d, u, dx); });
    }
}

// Scratch of the two-pass backward: the queries, then the pair sort's
struct Bwd2Scratch {
    size_t q_bytes, total;
    PairSortPlan sort;
};
static int bwd2_scratch(const mkb_tables_t *tb, int64_t B, int64_t K, Bwd2Scratch &S) {
    if (int rc = pair_sort_plan(tb->n_entity, B * K, S.sort)) return rc;
    S.q_bytes = ((size_t)B * tb->entity_dim * 4 + 255) & ~(size_t)255;
    S.total = S.q_bytes + S.sort.total;
    return MKB_OK;
}
static bool bwd2_applies(const mkb_tables_t *tb, const int64_t *cand, int64_t B, int64_t K) {
    return cand && K > 1 && B * K <= INT32_MAX && tb->n_entity <= INT32_MAX;
}

template <int MODEL, bool HEAD>
static int launch_bwd2(const TablesDev &T, const mkb_tables_t *tb, const mkb_grads_t &G, const int64_t *sample, const int64_t *cand,
                       int64_t B, int K, const float *dscore, void *ws, hipStream_t st) {
    const int64_t n = B * K;
    Bwd2Scratch S;
    if (int rc = bwd2_scratch(tb, B, K, S)) return rc;
    float *Q = (float *)ws;  // caller-owned (mkb_score_bwd_workspace_bytes): nothing is allocated here
    const int *sorted_cand, *sorted_pair;
    ProfScope ps(MKB_PROF_GENERAL_BWD, st);
    if (int rc = pair_sort_launch(cand, n, tb->n_entity, (unsigned char *)ws + S.q_bytes, S.sort, st, &sorted_cand, &sorted_pair)) return rc;
    const unsigned chunks = (unsigned)((n + kChunkPairs - 1) / kChunkPairs);
    static_assert(kBlock == 256, "query_build_kernel strides its row by 256 lanes");
    const RowArgs qa = query_build_args(T.ent, T.rel, sample, Q, T.De, T.Dr, T.d, B, T.kd);
    hipLaunchKernelGGL((query_build_kernel<MODEL, HEAD>), dim3((unsigned)B), dim3(kBlock), 0, st, qa);
    hipLaunchKernelGGL((score_bwd_kernel<MODEL, HEAD, false>), dim3((unsigned)B), dim3(kBlock), 0, st, T, G, sample, cand, K, dscore);
    hipLaunchKernelGGL((score_bwd_x_kernel<MODEL, HEAD>), dim3(chunks), dim3(kBlock), 0, st, T, G, sorted_cand, sorted_pair, (int)n, K, Q, dscore);
    MKB_LAUNCH_CHECK();
    return MKB_OK;
}

template <int MODEL, bool HEAD>
static int launch_fwd(const TablesDev &T, const int64_t *sample, const int64_t *cand, int64_t B, int K, float *score, hipStream_t st) {
    const size_t lds = (size_t)T.De * sizeof(float);
    ProfScope ps(MKB_PROF_GENERAL_FWD, st);
    hipLaunchKernelGGL((score_fwd_kernel<MODEL, HEAD>), dim3((unsigned)B), dim3(kBlock), lds, st, T, sample, cand, K, score);
    MKB_LAUNCH_CHECK();
    return MKB_OK;
}

template <int MODEL, bool HEAD>
static int launch_bwd(const TablesDev &T, const mkb_grads_t &G, const int64_t *sample, const int64_t *cand, int64_t B, int K,
                      const float *dscore, hipStream_t st) {
    ProfScope ps(MKB_PROF_GENERAL_BWD, st);
    hipLaunchKernelGGL((score_bwd_kernel<MODEL, HEAD, true>), dim3((unsigned)B), dim3(kBlock), 0, st, T, G, sample, cand, K, dscore);
    MKB_LAUNCH_CHECK();
    return MKB_OK;
}

static int check_call(const mkb_tables_t *tb, const int64_t *sample, const int64_t *cand, int64_t B, int64_t K, int mode) {
    if (int rc = validate_tables(tb)) return rc;
    MKB_REQUIRE(sample != nullptr && B >= 0 && K >= 1, "bad sample / B / K");
    MKB_REQUIRE(mode >= MKB_MODE_DEFAULT && mode <= MKB_MODE_TAIL, "bad mode %d", mode);
    MKB_REQUIRE(mode == MKB_MODE_DEFAULT ? (cand == nullptr && K == 1) : (cand != nullptr),
                "default mode takes no candidates (K=1); head/tail-batch need them");
    MKB_REQUIRE(tb->entity_dim * 4 <= 64 * 1024, "entity_dim too large for the LDS-staged query");
    MKB_REQUIRE(K <= INT32_MAX && B <= INT32_MAX, "B / K too large");
    return MKB_OK;
}

}  // namespace mkb

using namespace mkb;

extern "C" int mkb_score_fwd(const mkb_tables_t *tb, const int64_t *sample, const int64_t *cand, int64_t B, int64_t K,
                             int mode, float *score, void *stream) {
    if (int rc = check_call(tb, sample, cand, B, K, mode)) return rc;
    MKB_REQUIRE(score != nullptr, "score is null");
    if (B == 0) return MKB_OK;
    const TablesDev T = to_dev(tb);
    hipStream_t st = (hipStream_t)stream;
    return dispatch_model_side(tb->model, mode_is_head(mode), [&](auto m, auto h) {
        return launch_fwd<m(), h()>(T, sample, cand, B, (int)K, score, st);
    });
}

extern "C" int64_t mkb_score_bwd_workspace_bytes(const mkb_tables_t *tb, int64_t B, int64_t K, int mode) {
    if (!tb || B <= 0 || K <= 1 || mode == MKB_MODE_DEFAULT) return 0;
    if (B * K > INT32_MAX || tb->n_entity > INT32_MAX) return 0;  // (the one-pass kernel: no scratch)
    Bwd2Scratch S;
    return bwd2_scratch(tb, B, K, S) ? -1 : (int64_t)S.total;
}

extern "C" int mkb_score_bwd(const mkb_tables_t *tb, const mkb_grads_t *gr, const int64_t *sample, const int64_t *cand,
                             int64_t B, int64_t K, int mode, const float *dscore, void *ws, void *stream) {
    if (int rc = check_call(tb, sample, cand, B, K, mode)) return rc;
    MKB_REQUIRE(gr && gr->g_ent && gr->g_rel && dscore, "null gradient buffer");
    MKB_REQUIRE(tb->model != MKB_PROTATE || gr->g_modulus, "pRotatE needs g_modulus");
    if (B == 0) return MKB_OK;
    const TablesDev T = to_dev(tb);
    hipStream_t st = (hipStream_t)stream;
    const bool two_pass = bwd2_applies(tb, cand, B, K);
    MKB_REQUIRE(!two_pass || (ws != nullptr && (((uintptr_t)ws) & 255) == 0),
                "mkb_score_bwd needs a 256-byte aligned workspace of mkb_score_bwd_workspace_bytes() bytes");
    return dispatch_model_side(tb->model, mode_is_head(mode), [&](auto m, auto h) {
        return two_pass ? launch_bwd2<m(), h()>(T, tb, *gr, sample, cand, B, (int)K, dscore, ws, st)
                        : launch_bwd<m(), h()>(T, *gr, sample, cand, B, (int)K, dscore, st);
    });
}
