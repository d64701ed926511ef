// All-entity training for the distance models TransE / RotatE / pRotatE (include/mkb_hip.h, "all-entity losses, distance models"):
// the 1vsAll softmax, its filtered / label-smoothed form and the KvsAll multi-label BCE of score_all.hip, for a score that is not a
// product,
//     s_i(e) = finish_score(sum_k f(q_i[k], E[e][k]))      (model_math.h),
// so that the backward of the block cannot be two matrix products.
//
//   forward   run_rank (rank_all.h), as score_all.hip and the evaluation: the outer-product register tile for TransE / RotatE, the
//             lane-owns-dims kernel for pRotatE and for the shapes and pointers the tile does not take.  Where the route leaves raw pair
//             sums, dist_affine_kernel finishes them in place (S = c0 + c1 S): the loss kernels want scores.  ld = N on every route.
//   loss      the three loss kernels of score_all.hip, untouched (all_chain.h declares their launches); S becomes dS.
//   backward  the pair terms are recomputed, once per pass -- a second [B, N, De]-sized anything does not exist:
//       dist_dq_kernel  query-major.  A workgroup owns kDT = 16 query rows and 256 units of the row and walks a slice of the entities in
//                       order: a lane holds its unit of the 16 queries and their 16 sums in registers, loads the entity's unit
//                       (consecutive lanes, consecutive floats) and reads the 16 seeds of that entity from LDS (a [64 entities, 16]
//                       block of dS staged per 64 entities, one address for the whole wave: a broadcast).  With few row tiles the
//                       entities are split over grid.z (up to 8 slices, each a multiple of 64 entities) into partial buffers that
//                       dist_dq_reduce_kernel adds left to right.
//       dist_de_kernel  entity-major, the same tile turned round: a workgroup owns 16 entity rows and 256 units and walks ALL B queries
//                       in batch order; a lane holds its unit of the 16 entities and their 16 sums, loads the query's unit from Q and
//                       reads the 16 seeds of that query from LDS.  The finished sums are ADDED to g_ent, each element by one lane.
//                       pRotatE: every workgroup also leaves its sum of dS |sin z| in a buffer that dist_mod_kernel adds up in fixed
//                       order (256 contiguous segments left to right, then their totals left to right) and adds to g_modulus once.
//             Q needs no LDS staging in either pass: every element of Q (of E) a workgroup reads, it reads once, coalesced.  Every load
//             is a 4-byte load: tables at any alignment take the same path.  Rows or units past the end are clamped for the loads, get
//             seeds of exactly 0 and are not written.
//   chain     dQ -> the query's entity row and relation row: all_stash_kernel / all_chain_kernel over the radix-sorted occurrences
//             (all_chain.h), the very code of score_all.hip, for these three models.
// No float atomics: every gradient element has one writer and every sum a fixed order, so loss, dQ, both gradient tables and the
// modulus gradient have the same bits run to run, and a gradient buffer that held something ends as that + the step's result.
// The per-element derivatives and their edge conventions are model_math.h's: TransE's sign of an exact zero difference is 0,
// RotatE's clamped norm gives a coinciding pair a gradient of exactly 0.
// A single pass producing dQ and dE from one evaluation of the pair term was not tried: one of the two sums would have to leave
// the workgroup as a partial per tile ([N / 16, B, De] or [B / 16, N, De] floats) to keep the one-writer rule without atomics.
#include "common.h"
#include "all_chain.h"
#include "loss_math.h"  // block_sum_256
#include "rank_all.h"

#include <algorithm>

namespace mkb {

constexpr int kDT = 16;  // rows of the owned side per workgroup: 16 operand + 16 (RotatE: 32 + 32) sum registers per lane
constexpr int kDC = 64;  // rows of the walked side per staged block of dS: 4 KB of LDS
constexpr int kDqSlicesMax = 8, kDqTilesWanted = 1024;

struct DistArgs {
    const float *ent, *Q, *dS, *modulus;
    float *g_ent, *dQ, *modpart;  // dQ: [B, De], or the partials [slices, B, De]
    int B, d, U;                  // U: units per row (d for RotatE, De otherwise)
    int64_t N, De, ld, per;       // per: entities per slice of the dQ pass (a multiple of kDC)
    float kd;
};

// one pair: the seed g = d loss / d s_i(e) -> the unit's contributions to dq and dx; ex accumulates g |sin z| (pRotatE)
template <int MODEL, bool HEAD>
__device__ __forceinline__ void dist_pair_bwd(float q0, float q1, float x0, float x1, float g, float kd, float mod, float &dq0, float &dq1,
                                              float &dx0, float &dx1, float &ex) {
    if constexpr (ModelTraits<MODEL>::cplx_pair) {
        Cplx dq, dx;
        pair_bwd_cmod(Cplx{q0, q1}, Cplx{x0, x1}, g, dq, dx);
        dq0 = dq.re; dq1 = dq.im; dx0 = dx.re; dx1 = dx.im;
    } else {
        float e = 0.f;
        pair_bwd_real<MODEL, HEAD>(q0, x0, g, kd, mod, dq0, dx0, e);
        dq1 = dx1 = 0.f;
        ex += g * e;
    }
}

// grid (ceil(B / kDT), ceil(U / 256), slices)
template <int MODEL, bool HEAD>
__global__ __launch_bounds__(256) void dist_dq_kernel(DistArgs A) {
    constexpr bool CP = ModelTraits<MODEL>::cplx_pair;
    __shared__ __attribute__((aligned(16))) float s_g[kDC][kDT];
    const int tid = threadIdx.x;
    const int u = blockIdx.y * 256 + tid, uc = min(u, A.U - 1);
    const int i0 = blockIdx.x * kDT;
    const float mod = MODEL == MKB_PROTATE ? A.modulus[0] : 1.f;
    float q0[kDT], q1[kDT], a0[kDT], a1[kDT];
#pragma unroll
    for (int r = 0; r < kDT; ++r) {
        const float *q = A.Q + (int64_t)min(i0 + r, A.B - 1) * A.De;
        q0[r] = q[uc];
        q1[r] = CP ? q[A.d + uc] : 0.f;
        a0[r] = a1[r] = 0.f;
    }
    const int64_t e_lo = (int64_t)blockIdx.z * A.per, e_hi = min(A.N, e_lo + A.per);
    for (int64_t ec = e_lo; ec < e_hi; ec += kDC) {
        __syncthreads();
        for (int k = tid; k < kDC * kDT; k += 256) {
            const int r = k % kDT, c = k / kDT;
            s_g[c][r] = (i0 + r < A.B && ec + c < e_hi) ? A.dS[(int64_t)(i0 + r) * A.ld + ec + c] : 0.f;
        }
        __syncthreads();
#pragma unroll 2
        for (int c = 0; c < kDC; ++c) {
            const float *x = A.ent + min(ec + c, A.N - 1) * A.De;
            const float x0 = x[uc], x1 = CP ? x[A.d + uc] : 0.f;
            float g[kDT];
#pragma unroll
            for (int r = 0; r < kDT; r += 4) {
                const float4 v = *(const float4 *)&s_g[c][r];
                g[r] = v.x; g[r + 1] = v.y; g[r + 2] = v.z; g[r + 3] = v.w;
            }
#pragma unroll
            for (int r = 0; r < kDT; ++r) {
                float dq0, dq1, dx0, dx1, ex = 0.f;
                dist_pair_bwd<MODEL, HEAD>(q0[r], q1[r], x0, x1, g[r], A.kd, mod, dq0, dq1, dx0, dx1, ex);
                a0[r] += dq0;
                if constexpr (CP) a1[r] += dq1;
            }
        }
    }
    if (u >= A.U) return;
    float *out = A.dQ + (int64_t)blockIdx.z * A.B * A.De;
#pragma unroll
    for (int r = 0; r < kDT; ++r)
        if (i0 + r < A.B) {
            float *o = out + (int64_t)(i0 + r) * A.De;
            o[u] = a0[r];
            if constexpr (CP) o[A.d + u] = a1[r];
        }
}

// dQ[k] = part[0][k] + part[1][k] + ... left to right
static __global__ __launch_bounds__(256) void dist_dq_reduce_kernel(const float *__restrict__ part, float *__restrict__ dQ, int64_t n,
                                                                    int slices) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    float acc = part[k];
    for (int z = 1; z < slices; ++z) acc += part[(int64_t)z * n + k];
    dQ[k] = acc;
}

// grid (ceil(N / kDT), ceil(U / 256))
template <int MODEL, bool HEAD>
__global__ __launch_bounds__(256) void dist_de_kernel(DistArgs A) {
    constexpr bool CP = ModelTraits<MODEL>::cplx_pair;
    __shared__ __attribute__((aligned(16))) float s_g[kDC][kDT];
    __shared__ float red[4];
    const int tid = threadIdx.x;
    const int u = blockIdx.y * 256 + tid, uc = min(u, A.U - 1);
    const int64_t e0 = (int64_t)blockIdx.x * kDT;
    const float mod = MODEL == MKB_PROTATE ? A.modulus[0] : 1.f;
    float x0[kDT], x1[kDT], a0[kDT], a1[kDT];
#pragma unroll
    for (int j = 0; j < kDT; ++j) {
        const float *x = A.ent + min(e0 + j, A.N - 1) * A.De;
        x0[j] = x[uc];
        x1[j] = CP ? x[A.d + uc] : 0.f;
        a0[j] = a1[j] = 0.f;
    }
    float macc = 0.f;
    for (int ic = 0; ic < A.B; ic += kDC) {
        __syncthreads();
        for (int k = tid; k < kDC * kDT; k += 256) {
            const int j = k % kDT, c = k / kDT;
            s_g[c][j] = (ic + c < A.B && e0 + j < A.N) ? A.dS[(int64_t)(ic + c) * A.ld + e0 + j] : 0.f;
        }
        __syncthreads();
#pragma unroll 2
        for (int c = 0; c < kDC; ++c) {
            const float *q = A.Q + (int64_t)min(ic + c, A.B - 1) * A.De;
            const float q0 = q[uc], q1 = CP ? q[A.d + uc] : 0.f;
            float g[kDT];
#pragma unroll
            for (int j = 0; j < kDT; j += 4) {
                const float4 v = *(const float4 *)&s_g[c][j];
                g[j] = v.x; g[j + 1] = v.y; g[j + 2] = v.z; g[j + 3] = v.w;
            }
#pragma unroll
            for (int j = 0; j < kDT; ++j) {
                float dq0, dq1, dx0, dx1;
                dist_pair_bwd<MODEL, HEAD>(q0, q1, x0[j], x1[j], g[j], A.kd, mod, dq0, dq1, dx0, dx1, macc);
                a0[j] += dx0;
                if constexpr (CP) a1[j] += dx1;
            }
        }
    }
    if (u < A.U) {
#pragma unroll
        for (int j = 0; j < kDT; ++j)
            if (e0 + j < A.N) {
                float *o = A.g_ent + (e0 + j) * A.De;
                o[u] += a0[j];
                if constexpr (CP) o[A.d + u] += a1[j];
            }
    }
    if constexpr (MODEL == MKB_PROTATE) {
        if (A.modpart) {  // (uniform)
            const float t = block_sum_256(u < A.U ? macc : 0.f, red);
            if (tid == 0) A.modpart[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = t;
        }
    }
}

// g_modulus[0] += -(part[0] + ... + part[n - 1]): lane l adds its contiguous segment left to right, lane 0 the 256 totals left to right
static __global__ __launch_bounds__(256) void dist_mod_kernel(const float *__restrict__ part, int64_t n, float *__restrict__ g_modulus) {
    __shared__ float s_tot[256];
    const int64_t per = (n + 255) / 256, lo = threadIdx.x * per, hi = min(n, lo + per);
    float acc = 0.f;
    for (int64_t k = lo; k < hi; ++k) acc += part[k];
    s_tot[threadIdx.x] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        float t = 0.f;
        for (int l = 0; l < 256; ++l) t += s_tot[l];
        g_modulus[0] += -t;
    }
}

// S[i, e] = c0 + c1 S[i, e] over the first N columns of each row: raw pair sums -> scores (export_scores_kernel's expression)
static __global__ __launch_bounds__(256) void dist_affine_kernel(float *__restrict__ S, int64_t N, int64_t ld, float c0, float c1) {
    const int64_t i = blockIdx.y;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < N; e += (int64_t)gridDim.x * 256) S[i * ld + e] = c0 + c1 * S[i * ld + e];
}

// ---- workspace: Q [B, De], the score block [B, Npad] (which becomes dS), the id list [Npad], dQ [B, De], the stash [B, De] of
// all_stash_kernel, the dQ pass's partials [slices, B, De], the sort's storage, the loss scratch [1 + B], the
// modulus partials (pRotatE: one float per workgroup of the dE pass)
struct DistPlan {
    PairSortPlan sort;
    int slices, uslices;
    int64_t per, de_tiles;
    size_t s_off, ids_off, dq_off, stash_off, part_off, sort_off, scr_off, mod_off, total;
};
struct DistWs {
    float *Q, *S;
    int64_t *ids;
    float *dQ, *stash, *part;
    void *sort;
    float *scratch, *modpart;
};

static int64_t dist_units(const mkb_tables_t *tb) { return tb->model == MKB_ROTATE ? tb->hidden_dim : tb->entity_dim; }

// The shapes of all_plan (score_all.hip): one int32 sort and B * Npad, B * De below 2^31 (B >= 1 is the caller's).  false: outside
// them, or the sort's size query failed (*rc < 0)
static bool dist_plan(const mkb_tables_t *tb, int64_t B, DistPlan &P, int *rc) {
    *rc = 0;
    const int64_t N = tb->n_entity, Npad = all_npad(N), De = tb->entity_dim;
    if (N <= 0 || tb->n_relation <= 0 || De <= 0 || Npad >= (1 << 30) || N + tb->n_relation > INT32_MAX || B > INT32_MAX / 2 ||
        B * Npad > INT32_MAX || B * De > INT32_MAX)
        return false;
    if ((*rc = pair_sort_plan(N + tb->n_relation, 2 * B, P.sort))) return false;
    P.uslices = (int)((dist_units(tb) + 255) / 256);
    P.de_tiles = (N + kDT - 1) / kDT;
    // the dQ pass: enough workgroups to fill the device, every slice a multiple of the staged block
    const int64_t tiles = (B + kDT - 1) / kDT * P.uslices, blocks = (N + kDC - 1) / kDC;
    const int64_t want = std::min<int64_t>(std::min<int64_t>((kDqTilesWanted + tiles - 1) / tiles, kDqSlicesMax), blocks);
    P.per = (blocks + want - 1) / want * kDC;
    P.slices = (int)((N + P.per - 1) / P.per);
    P.s_off = up256((size_t)B * De * 4);
    P.ids_off = P.s_off + up256((size_t)B * Npad * 4);
    P.dq_off = P.ids_off + up256((size_t)Npad * 8);
    P.stash_off = P.dq_off + up256((size_t)B * De * 4);
    P.part_off = P.stash_off + up256((size_t)B * De * 4);
    // the partials, sized by a bound that grows with B where slices * B itself does not: slices <= 8 and slices <= 1024 / tiles + 1
    // with tiles >= B uslices / 16
    const int64_t part_rows = std::min<int64_t>(kDqSlicesMax * B, (int64_t)kDqTilesWanted * kDT / P.uslices + B);
    P.sort_off = P.part_off + up256((size_t)part_rows * De * 4);
    P.scr_off = P.sort_off + P.sort.total;
    P.mod_off = P.scr_off + up256((size_t)(B + 1) * 4);
    P.total = P.mod_off + (tb->model == MKB_PROTATE ? up256((size_t)P.de_tiles * P.uslices * 4) : 0);
    return true;
}

static DistWs dist_carve(const DistPlan &P, void *ws) {
    unsigned char *b = (unsigned char *)ws;
    return DistWs{(float *)b, (float *)(b + P.s_off), (int64_t *)(b + P.ids_off), (float *)(b + P.dq_off), (float *)(b + P.stash_off),
                  (float *)(b + P.part_off), b + P.sort_off, (float *)(b + P.scr_off), (float *)(b + P.mod_off)};
}

static bool dist_model(int model) { return model == MKB_TRANSE || model == MKB_ROTATE || model == MKB_PROTATE; }

// dispatch_model_side (common.h) for the three distance models; ComplEx and DistMult are sent to their own calls
template <class F>
static int dispatch_dist_model(int model, bool head, F &&f) {
    if (!dist_model(model))
        return set_error(MKB_ERR_UNSUPPORTED,
                         "the mkb_dist_all_* calls cover TransE, RotatE and pRotatE; ComplEx and DistMult, whose all-entity block is one "
                         "matrix product, have mkb_all_step, mkb_all_kvs_step, mkb_all_filtered_step and mkb_all_score_fwd / _bwd");
    return dispatch_model_side(model, head, [&](auto m, auto h) {  // (no kernels are instantiated for the models refused above)
        if constexpr (decltype(m)::value == MKB_TRANSE || decltype(m)::value == MKB_ROTATE || decltype(m)::value == MKB_PROTATE) return f(m, h);
        else return (int)MKB_ERR_UNSUPPORTED;
    });
}

// what every entry point that takes tables, a batch and the workspace checks, in the order of score_all.hip's all_check
static int dist_check(const mkb_tables_t *tb, const int64_t *sample, int64_t B, int mode, const void *ws, int64_t ws_bytes, DistPlan &P) {
    if (int rc = validate_tables(tb)) return rc;
    MKB_REQUIRE(sample && ws, "null pointer");
    MKB_REQUIRE(mode == MKB_MODE_HEAD || mode == MKB_MODE_TAIL, "the all-entity losses need head-batch or tail-batch");
    MKB_REQUIRE(B >= 1, "B must be >= 1");
    if (!dist_model(tb->model)) return dispatch_dist_model(tb->model, false, [](auto, auto) { return MKB_OK; });
    MKB_REQUIRE(tb->entity_dim <= 4 * kWGr, "rows of more than 4096 units are not supported");
    int rc;
    if (!dist_plan(tb, B, P, &rc)) {
        if (rc) return rc;
        MKB_REQUIRE(false, "B * (n_entity + 3) and B * entity_dim must stay below 2^31, n_entity below 2^30");
    }
    MKB_REQUIRE(ws_bytes >= (int64_t)P.total && (((uintptr_t)ws) & 255) == 0, "workspace too small / unaligned");
    return MKB_OK;
}

// dS [B, ld] -> g_ent, g_rel, g_modulus (accumulated).  w.Q holds the batch's queries.
template <int MODEL, bool HEAD>
static int dist_bwd(const mkb_tables_t *tb, const mkb_grads_t *gr, const int64_t *sample, int64_t B, const float *dS, int64_t ld,
                    const DistPlan &P, const DistWs &w, hipStream_t st) {
    const int64_t N = tb->n_entity, De = tb->entity_dim;
    ChainArgs C;
    if (int rc = all_chain_open<HEAD>(tb, gr, sample, B, w.dQ, w.stash, w.sort, P.sort, st, C)) return rc;
    DistArgs A{};
    A.ent = tb->ent; A.Q = w.Q; A.dS = dS; A.modulus = tb->modulus; A.g_ent = gr->g_ent;
    A.dQ = P.slices > 1 ? w.part : w.dQ;
    A.modpart = MODEL == MKB_PROTATE && gr->g_modulus ? w.modpart : nullptr;
    A.B = (int)B; A.d = tb->hidden_dim; A.U = (int)dist_units(tb); A.N = N; A.De = De; A.ld = ld; A.per = P.per; A.kd = tb->phase_div;
    hipLaunchKernelGGL((dist_dq_kernel<MODEL, HEAD>), dim3((unsigned)((B + kDT - 1) / kDT), (unsigned)P.uslices, (unsigned)P.slices), dim3(256),
                       0, st, A);
    if (P.slices > 1)
        hipLaunchKernelGGL(dist_dq_reduce_kernel, dim3((unsigned)((B * De + 255) / 256)), dim3(256), 0, st, w.part, w.dQ, B * De, P.slices);
    hipLaunchKernelGGL((dist_de_kernel<MODEL, HEAD>), dim3((unsigned)P.de_tiles, (unsigned)P.uslices), dim3(256), 0, st, A);
    if (A.modpart) hipLaunchKernelGGL(dist_mod_kernel, dim3(1), dim3(256), 0, st, w.modpart, P.de_tiles * P.uslices, gr->g_modulus);
    hipLaunchKernelGGL((all_chain_kernel<MODEL, HEAD>), dim3((unsigned)(2 * B)), dim3(256), 0, st, C);
    MKB_LAUNCH_CHECK();
    return MKB_OK;
}

// The step behind mkb_dist_all_step, mkb_dist_all_kvs_step and mkb_dist_all_filtered_step, whose checks have passed: the forward
// block, finished where the route left raw pair sums, the loss on it -- loss(S, ld, scratch) leaves dS in S --, the backward.
template <class Loss>
static int dist_step(const mkb_tables_t *tb, const mkb_grads_t *gr, const int64_t *sample, int64_t B, int mode, const DistPlan &P, void *ws,
                     hipStream_t st, Loss &&loss) {
    const DistWs w = dist_carve(P, ws);
    const int64_t N = tb->n_entity;
    int64_t ld_S = 0;
    auto finish = [&](float c0, float c1, int64_t ld) {
        ld_S = ld;
        if (!(c0 == 0.f && c1 == 1.f))
            hipLaunchKernelGGL(dist_affine_kernel, dim3((unsigned)std::min<int64_t>((N + 255) / 256, 64), (unsigned)B), dim3(256), 0, st, w.S, N,
                               ld, c0, c1);
        loss(w.S, ld, w.scratch);
    };
    return dispatch_dist_model(tb->model, mode == MKB_MODE_HEAD, [&](auto m, auto h) {
        if (int rc = run_rank<m(), h()>(tb, sample, B, w.Q, w.S, w.ids, st, finish)) return rc;
        return dist_bwd<m(), h()>(tb, gr, sample, B, w.S, ld_S, P, w, st);
    });
}

}  // namespace mkb

using namespace mkb;

extern "C" int64_t mkb_dist_all_workspace_bytes(const mkb_tables_t *tb, int64_t B) {
    DistPlan P;
    int rc;
    if (!tb || B <= 0 || !dist_model(tb->model) || !dist_plan(tb, B, P, &rc)) return 0;
    return (int64_t)P.total;
}

extern "C" int mkb_dist_all_score_fwd(const mkb_tables_t *tb, const int64_t *sample, int64_t B, int mode, float *scores, void *ws,
                                      int64_t ws_bytes, void *stream) {
    DistPlan P;
    MKB_REQUIRE(scores, "null pointer");
    if (int rc = dist_check(tb, sample, B, mode, ws, ws_bytes, P)) return rc;
    const DistWs w = dist_carve(P, ws);
    hipStream_t st = (hipStream_t)stream;
    auto finish = [&](float f0, float f1, int64_t ld) {  // the evaluation's export: the bits mkb_rank_scores hands out
        hipLaunchKernelGGL(export_scores_kernel, dim3((unsigned)std::min<int64_t>((tb->n_entity + 255) / 256, 64), (unsigned)B), dim3(256), 0,
                           st, w.S, scores, tb->n_entity, ld, f0, f1);
    };
    return dispatch_dist_model(tb->model, mode == MKB_MODE_HEAD,
                               [&](auto m, auto h) { return run_rank<m(), h()>(tb, sample, B, w.Q, w.S, w.ids, st, finish); });
}

extern "C" int mkb_dist_all_score_bwd(const mkb_tables_t *tb, const mkb_grads_t *gr, const int64_t *sample, int64_t B, int mode,
                                      const float *dscore, int64_t ld, void *ws, int64_t ws_bytes, void *stream) {
    DistPlan P;
    MKB_REQUIRE(gr && gr->g_ent && gr->g_rel && dscore, "null pointer");
    if (int rc = dist_check(tb, sample, B, mode, ws, ws_bytes, P)) return rc;
    MKB_REQUIRE(ld >= tb->n_entity && B * ld <= INT32_MAX, "need ld >= n_entity and B * ld below 2^31");
    const DistWs w = dist_carve(P, ws);
    hipStream_t st = (hipStream_t)stream;
    return dispatch_dist_model(tb->model, mode == MKB_MODE_HEAD, [&](auto m, auto h) {
        const RowArgs ra = query_build_args(tb->ent, tb->rel, sample, w.Q, tb->entity_dim, tb->relation_dim, tb->hidden_dim, B, tb->phase_div);
        hipLaunchKernelGGL((query_build_kernel<m(), h()>), dim3((unsigned)B), dim3(256), 0, st, ra);
        return dist_bwd<m(), h()>(tb, gr, sample, B, dscore, ld, P, w, st);
    });
}

extern "C" int mkb_dist_all_step(const mkb_tables_t *tb, const mkb_grads_t *gr, const int64_t *sample, const float *weight, int64_t B,
                                 int mode, float temperature, const float *weight_sum, float *loss, float *pos, void *ws,
                                 int64_t ws_bytes, void *stream) {
    DistPlan P;
    MKB_REQUIRE(gr && gr->g_ent && gr->g_rel && loss && pos, "null pointer");
    MKB_REQUIRE(temperature - temperature == 0.f && temperature > 0.f, "the softmax temperature must be finite and > 0");
    if (int rc = dist_check(tb, sample, B, mode, ws, ws_bytes, P)) return rc;
    hipStream_t st = (hipStream_t)stream;
    return dist_step(tb, gr, sample, B, mode, P, ws, st, [&](float *S, int64_t ld, float *scratch) {
        all_softmax_launch(S, B, tb->n_entity, ld, sample + (mode == MKB_MODE_HEAD ? 0 : 2), 3, weight, weight_sum, temperature, loss, pos,
                           scratch, st);
    });
}

extern "C" int mkb_dist_all_kvs_step(const mkb_tables_t *tb, const mkb_grads_t *gr, const int64_t *sample, const float *weight, int64_t B,
                                     int mode, const int64_t *keys, int64_t n_keys, float smoothing, int sum_over_entities,
                                     const float *weight_sum, float *loss, float *pos, void *ws, int64_t ws_bytes, void *stream) {
    DistPlan P;
    MKB_REQUIRE(gr && gr->g_ent && gr->g_rel && loss && pos, "null pointer");
    if (int rc = dist_check(tb, sample, B, mode, ws, ws_bytes, P)) return rc;
    if (int rc = bce_check(tb->n_entity, tb->n_relation, mode, keys, n_keys, smoothing)) return rc;
    hipStream_t st = (hipStream_t)stream;
    return dist_step(tb, gr, sample, B, mode, P, ws, st, [&](float *S, int64_t ld, float *scratch) {
        all_bce_launch(S, B, tb->n_entity, ld, sample, mode == MKB_MODE_HEAD, tb->n_relation, keys, n_keys, weight, weight_sum, smoothing,
                       sum_over_entities != 0, loss, pos, scratch, st);
    });
}

extern "C" int mkb_dist_all_filtered_step(const mkb_tables_t *tb, const mkb_grads_t *gr, const int64_t *sample, const float *weight,
                                          int64_t B, int mode, const int64_t *keys, int64_t n_keys, float T, float smoothing,
                                          const float *weight_sum, float *loss, float *pos, void *ws, int64_t ws_bytes, void *stream) {
    DistPlan P;
    MKB_REQUIRE(gr && gr->g_ent && gr->g_rel && loss && pos, "null pointer");
    MKB_REQUIRE(T - T == 0.f && T > 0.f, "the softmax temperature must be finite and > 0");
    if (int rc = dist_check(tb, sample, B, mode, ws, ws_bytes, P)) return rc;
    if (int rc = bce_check(tb->n_entity, tb->n_relation, mode, keys, n_keys, smoothing, "filtered 1vsAll")) return rc;
    hipStream_t st = (hipStream_t)stream;
    return dist_step(tb, gr, sample, B, mode, P, ws, st, [&](float *S, int64_t ld, float *scratch) {
        all_softmax_filtered_launch(S, B, tb->n_entity, ld, sample + (mode == MKB_MODE_HEAD ? 0 : 2), 3, sample, mode == MKB_MODE_HEAD,
                                    tb->n_relation, keys, n_keys, weight, weight_sum, T, smoothing, loss, pos, scratch, st);
    });
}
