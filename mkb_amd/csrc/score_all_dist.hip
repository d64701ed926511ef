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
// The host side -- workspace plan, entry checks, model dispatch, the step and the bodies of the calls -- is all_host.h's, shared with
// score_all.hip; this file gives it DistFamily: the three models, the two passes' launch fields and buffers, the affine finish and
// the backward above.
#include "common.h"
#include "all_host.h"   // (all_chain.h, rank_all.h)
#include "loss_math.h"  // block_sum_256

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

static int64_t dist_units(const mkb_tables_t *tb) { return tb->model == MKB_ROTATE ? tb->hidden_dim : tb->entity_dim; }

// ---- the family of the three distance models, for the protocol of all_host.h
struct DistFamily {
    static constexpr bool covers(int model) { return model == MKB_TRANSE || model == MKB_ROTATE || model == MKB_PROTATE; }
    static constexpr const char *refusal =
        "the mkb_dist_all_* calls cover TransE, RotatE and pRotatE; ComplEx and DistMult, whose all-entity block is one "
        "matrix product, have mkb_all_step, mkb_all_kvs_step, mkb_all_filtered_step and mkb_all_score_fwd / _bwd";
    static constexpr const char *mode_text = "the all-entity losses need head-batch or tail-batch";
    struct Launch {
        int slices, uslices;
        int64_t per, de_tiles;
    };

    // the dQ pass's partials [slices, B, De]; behind the loss scratch the modulus partials (pRotatE: one float per workgroup of the
    // dE pass)
    static FamilyBytes plan(const mkb_tables_t *tb, int64_t B, Launch &L) {
        const int64_t N = tb->n_entity, De = tb->entity_dim;
        L.uslices = (int)((dist_units(tb) + 255) / 256);
        L.de_tiles = (N + kDT - 1) / kDT;
        // the dQ pass: enough workgroups to fill the device, every slice a multiple of the staged block
        const int64_t tiles = (B + kDT - 1) / kDT * L.uslices, blocks = (N + kDC - 1) / kDC;
        const int64_t want = std::min<int64_t>(std::min<int64_t>((kDqTilesWanted + tiles - 1) / tiles, kDqSlicesMax), blocks);
        L.per = (blocks + want - 1) / want * kDC;
        L.slices = (int)((N + L.per - 1) / L.per);
        // the partials, sized by a bound that grows with B where slices * B itself does not: slices <= 8 and slices <= 1024 / tiles + 1
        // with tiles >= B uslices / 16
        const int64_t part_rows = std::min<int64_t>(kDqSlicesMax * B, (int64_t)kDqTilesWanted * kDT / L.uslices + B);
        return FamilyBytes{(size_t)part_rows * De * 4, tb->model == MKB_PROTATE ? (size_t)L.de_tiles * L.uslices * 4 : 0};
    }

    // raw pair sums -> scores: the loss kernels want scores
    static void finish_block(float *S, int64_t B, int64_t N, int64_t ld, float c0, float c1, hipStream_t st) {
        hipLaunchKernelGGL(dist_affine_kernel, dim3((unsigned)std::min<int64_t>((N + 255) / 256, 64), (unsigned)B), dim3(256), 0, st, S, N, ld,
                           c0, c1);
    }

    // dS [B, ld] -> g_ent, g_rel, g_modulus (accumulated); w.tail: the modulus partials
    template <int MODEL, bool HEAD>
    static int bwd(const mkb_tables_t *tb, const mkb_grads_t *gr, const int64_t *sample, int64_t B, const float *dS, int64_t ld, bool,
                   const AllPlan<DistFamily> &P, const AllWs &w, hipStream_t st) {
        const int64_t N = tb->n_entity, De = tb->entity_dim;
        const Launch &L = P.launch;
        ChainArgs C;
        if (int rc = all_chain_open<HEAD>(tb, gr, sample, B, w.dQ, w.stash, w.sort, P.sort, st, C)) return rc;
        DistArgs A{};
        A.ent = tb->ent; A.Q = w.Q; A.dS = dS; A.modulus = tb->modulus; A.g_ent = gr->g_ent;
        A.dQ = L.slices > 1 ? w.part : w.dQ;
        A.modpart = MODEL == MKB_PROTATE && gr->g_modulus ? w.tail : nullptr;
        A.B = (int)B; A.d = tb->hidden_dim; A.U = (int)dist_units(tb); A.N = N; A.De = De; A.ld = ld; A.per = L.per; A.kd = tb->phase_div;
        hipLaunchKernelGGL((dist_dq_kernel<MODEL, HEAD>), dim3((unsigned)((B + kDT - 1) / kDT), (unsigned)L.uslices, (unsigned)L.slices), dim3(256),
                           0, st, A);
        if (L.slices > 1)
            hipLaunchKernelGGL(dist_dq_reduce_kernel, dim3((unsigned)((B * De + 255) / 256)), dim3(256), 0, st, w.part, w.dQ, B * De, L.slices);
        hipLaunchKernelGGL((dist_de_kernel<MODEL, HEAD>), dim3((unsigned)L.de_tiles, (unsigned)L.uslices), dim3(256), 0, st, A);
        if (A.modpart) hipLaunchKernelGGL(dist_mod_kernel, dim3(1), dim3(256), 0, st, w.tail, L.de_tiles * L.uslices, gr->g_modulus);
        hipLaunchKernelGGL((all_chain_kernel<MODEL, HEAD>), dim3((unsigned)(2 * B)), dim3(256), 0, st, C);
        MKB_LAUNCH_CHECK();
        return MKB_OK;
    }
};

}  // namespace mkb

using namespace mkb;

// (the bodies of all_host.h for DistFamily)
extern "C" int64_t mkb_dist_all_workspace_bytes(const mkb_tables_t *tb, int64_t B) { return all_workspace_bytes<DistFamily>(tb, B); }

extern "C" int mkb_dist_all_score_fwd(const mkb_tables_t *tb, const int64_t *sample, int64_t B, int mode, float *scores, void *ws,
                                      int64_t ws_bytes, void *stream) {
    return all_score_fwd<DistFamily>(tb, sample, B, mode, scores, ws, ws_bytes, stream);
}

extern "C" int mkb_dist_all_score_bwd(const mkb_tables_t *tb, const mkb_grads_t *gr, const int64_t *sample, int64_t B, int mode,
                                      const float *dscore, int64_t ld, void *ws, int64_t ws_bytes, void *stream) {
    return all_score_bwd<DistFamily>(tb, gr, sample, B, mode, dscore, ld, ws, ws_bytes, stream);
}

extern "C" int mkb_dist_all_step(const mkb_tables_t *tb, const mkb_grads_t *gr, const int64_t *sample, const float *weight, int64_t B,
                                 int mode, float temperature, const float *weight_sum, float *loss, float *pos, void *ws,
                                 int64_t ws_bytes, void *stream) {
    return all_softmax_step<DistFamily>(tb, gr, sample, weight, B, mode, temperature, weight_sum, loss, pos, ws, ws_bytes, stream);
}

extern "C" int mkb_dist_all_kvs_step(const mkb_tables_t *tb, const mkb_grads_t *gr, const int64_t *sample, const float *weight, int64_t B,
                                     int mode, const int64_t *keys, int64_t n_keys, float smoothing, int sum_over_entities,
                                     const float *weight_sum, float *loss, float *pos, void *ws, int64_t ws_bytes, void *stream) {
    return all_kvs_step<DistFamily>(tb, gr, sample, weight, B, mode, keys, n_keys, smoothing, sum_over_entities, weight_sum, loss, pos, ws,
                                    ws_bytes, stream);
}

extern "C" int mkb_dist_all_filtered_step(const mkb_tables_t *tb, const mkb_grads_t *gr, const int64_t *sample, const float *weight,
                                          int64_t B, int mode, const int64_t *keys, int64_t n_keys, float T, float smoothing,
                                          const float *weight_sum, float *loss, float *pos, void *ws, int64_t ws_bytes, void *stream) {
    return all_filtered_step<DistFamily>(tb, gr, sample, weight, B, mode, keys, n_keys, T, smoothing, weight_sum, loss, pos, ws, ws_bytes,
                                         stream);
}
