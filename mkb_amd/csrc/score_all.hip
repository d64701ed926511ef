// 1vsAll softmax training for ComplEx / DistMult (include/mkb_hip.h, "1vsAll"): every entity is scored for each (h, r, ?) -- or
// (?, r, t) -- and the cross entropy is taken over the whole row,
//     row_i = log sum_{e < N} exp(s_i(e) / T) - s_i(target_i) / T,     loss = sum_i w_i row_i / W.
//
//   forward   the all-entity block of the evaluation (run_rank, rank_all.h): ONE matrix-core product S = Q . E^T, or the
//             lane-owns-dims kernel for the shapes that product does not take.  The route is chosen there, not here.
//   softmax   all_softmax_kernel: one 256-lane workgroup per row, three passes (maximum, partition sum, seeds); rows of up to
//             kAllStageCols columns are read once and kept in LDS, longer ones are re-read from global memory.  S is overwritten in
//             place with dS_ij = (w_i / (W T)) (p_ij - [j = target_i]); the columns N .. ld - 1 that the forward's padding fills
//             with the last entity's score take no part in the sums and their dS is written as exactly 0.
//   backward  dQ [B, De] = dS . E and dE [N, De] += dS^T . Q, both planned by plan_gemm (shapes and limits: all_plan.h) and launched
//             through launch_gemm; dE uses the accumulating epilogue (GEMM_ACCUM: every entity row is written by exactly one tile,
//             a K split is reduced in fixed order and the finished product added once).  Then dQ is chained into the query's
//             entity row and relation row (query_side.h): the 2 B occurrences are radix-sorted by row (pair_sort.h) and each
//             distinct row has a single writer that walks its occurrences in batch order and adds the sum onto the gradient row
//             (a query entity's row: together with its row of dE, in one rounded addition -- all_stash_kernel).
// No float atomics anywhere: loss and both gradient tables have the same bits run to run, and gradient buffers that held
// something end as that + the step's result, bit for bit.
// KvsAll (include/mkb_hip.h, "KvsAll") is the same step around another loss kernel, all_bce_kernel: the multi-label binary cross
// entropy with label smoothing, its labels read from the sorted key arrays of the filtered ranking.
// Filtered 1vsAll (include/mkb_hip.h, "filtered 1vsAll") is the third loss kernel, all_softmax_filtered_kernel: the softmax with a
// row's other known answers -- the same key range -- taken out of the row, and label smoothing over the columns that stay.
// Written once for the three: the launch of "a loss kernel on the block" (all_loss_launch), which runs it inside the row-loss
// protocol of loss_math.h (RowLoss: W, the scratch, the launch in front of many rows, the finish).
// Everything on the host around the kernels -- workspace plan, entry checks, model dispatch, the step (carve, forward, the loss on
// the block, backward) and the bodies of the calls that take tables -- is all_host.h's, shared with score_all_dist.hip, the same
// three losses for TransE / RotatE / pRotatE; this file gives it DotFamily: the two models, the partial buffer's size and the
// backward of the block.  all_chain.h declares the loss launches and holds the query chain.
#include "common.h"
#include "all_host.h"  // (all_chain.h, pair_sort.h, rank_all.h)
#include "loss_math.h"
#include "sampler_draw.h"  // lower_bound_dev
#include "score_row.h"     // table_row

#include <algorithm>
#include <math.h>

namespace mkb {

constexpr int kAllStageCols = 4096;  // 16 KB of LDS per row

// max over the workgroup's 256 lanes; every lane gets it.  red: 4 floats of LDS.
__device__ __forceinline__ float block_max_256(float v, float *red) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

// scal / scal_out / rowpart: the row-loss protocol (RowLoss, row_loss_weight_sum)
__global__ __launch_bounds__(256) void all_softmax_kernel(float *__restrict__ S, int B, int64_t N, int64_t ld,
                                                          const int64_t *__restrict__ target, int64_t tstride,
                                                          const float *__restrict__ w, const float *__restrict__ scal,
                                                          float *__restrict__ scal_out, float inv_T, float *__restrict__ pos,
                                                          float *__restrict__ rowpart) {
    __shared__ float red[4];
    extern __shared__ float s_row[];
    const int tid = threadIdx.x;
    const int64_t i = blockIdx.x;
    float *row = S + i * ld;
    const bool staged = N <= kAllStageCols;
    const int64_t t = table_row(target[i * tstride], N);  // (an id outside the table: the glue flags it, mkb_check_ids)
    const float p_i = row[t];  // before anything is overwritten: every lane reads it here, the barriers below come first
    const float wi = w ? w[i] : 1.f;

    float m = -INFINITY;
    for (int64_t j = tid; j < N; j += 256) {
        const float v = row[j];
        m = fmaxf(m, v);
        if (staged) s_row[j] = v;
    }
    const float W = row_loss_weight_sum(scal, scal_out, w, B, red);
    m = block_max_256(m, red);

    // every exponent relative to the row maximum in score units: the row is (m - pos) / T + log Z with Z >= 1
    float z = 0.f;
    for (int64_t j = tid; j < N; j += 256) {
        const float e = expf(((staged ? s_row[j] : row[j]) - m) * inv_T);
        z += e;
        if (staged) s_row[j] = e;
    }
    z = block_sum_256(z, red);  // lane-strided partial sums, then the fixed tree
    const float inv = 1.f / z, coef = wi * inv_T / W;
    for (int64_t j = tid; j < N; j += 256) {
        const float e = staged ? s_row[j] : expf((row[j] - m) * inv_T);
        row[j] = coef * (e * inv - (j == t ? 1.f : 0.f));
    }
    for (int64_t j = N + tid; j < ld; j += 256) row[j] = 0.f;  // the forward's pad columns
    if (tid == 0) {
        pos[i] = p_i;
        rowpart[i] = wi * ((m - p_i) * inv_T + logf(z));
    }
}

// A loss kernel on the block inside the row-loss protocol: run(L) launches it with L.scal_in, L.scal_out and L.rowpart
template <class Run>
static void all_loss_launch(const float *weight, const float *weight_sum, int64_t B, float *loss, float *scratch, hipStream_t st, Run &&run) {
    const RowLoss L = RowLoss::open(weight, weight_sum, B, scratch, st);
    run(L);
    L.finish(B, 1.f, loss, st);
}

void all_softmax_launch(float *S, int64_t B, int64_t N, int64_t ld, const int64_t *target, int64_t tstride, const float *weight,
                               const float *weight_sum, float T, float *loss, float *pos, float *scratch, hipStream_t st) {
    all_loss_launch(weight, weight_sum, B, loss, scratch, st, [&](const RowLoss &L) {
        const size_t lds = N <= kAllStageCols ? (size_t)N * sizeof(float) : 0;
        hipLaunchKernelGGL(all_softmax_kernel, dim3((unsigned)B), dim3(256), lds, st, S, (int)B, N, ld, target, tstride, weight, L.scal_in,
                           L.scal_out, 1.f / T, pos, L.rowpart);
    });
}

// ---- KvsAll (include/mkb_hip.h, "KvsAll"): multi-label binary cross entropy over the whole row, labels smoothed by eps,
//     y_ij = (1 - eps) [j in A_i] + eps / N,   row_i = c sum_{j < N} (softplus(s_ij) - y_ij s_ij),   dS_ij = (w_i c / W) (sigmoid(s_ij) - y_ij)
// A_i: the keys of the row's query q = e R + r (e: the head; the tail for head-batch) in the sorted key array of its side
// (utils/true_keys.py), the contiguous range [q N, (q + 1) N); label column = key - q N.  One 256-lane workgroup per row, no LDS
// staging (every column is read once and written once): the label columns' scores are summed BEFORE anything is overwritten, one
// dense pass writes coef (sigmoid(s) - eps / N), one sparse pass takes coef (1 - eps) off the label columns (keys are unique: one
// writer per element).  scal / scal_out / rowpart: as for all_softmax_kernel.
__global__ __launch_bounds__(256) void all_bce_kernel(float *__restrict__ S, int B, int64_t N, int64_t ld, const int64_t *__restrict__ sample,
                                                      int head, int64_t R, const int64_t *__restrict__ keys, int64_t n_keys,
                                                      const float *__restrict__ w, const float *__restrict__ scal,
                                                      float *__restrict__ scal_out, float eps, float c, float *__restrict__ pos,
                                                      float *__restrict__ rowpart) {
    __shared__ float red[4];
    const int tid = threadIdx.x;
    const int64_t i = blockIdx.x;
    float *row = S + i * ld;
    const int64_t *s = sample + 3 * i;
    // (an id outside its table counts as the nearest row, so that no label column leaves the row: the glue flags it, mkb_check_ids)
    const int64_t q = table_row(s[head ? 2 : 0], N) * R + table_row(s[1], R), base = q * N;
    const int64_t t = table_row(s[head ? 0 : 2], N);
    const int64_t lo = lower_bound_dev(keys, n_keys, base), hi = lower_bound_dev(keys, n_keys, base + N);  // (uniform; empty: lo == hi)
    const float p_i = row[t];  // before anything is overwritten: every lane reads it here, the barriers below come first
    const float wi = w ? w[i] : 1.f;

    float lab = 0.f;
    for (int64_t k = lo + tid; k < hi; k += 256) lab += row[table_row(keys[k] - base, N)];
    const float W = row_loss_weight_sum(scal, scal_out, w, B, red);
    lab = block_sum_256(lab, red);  // lane-strided partial sums, then the fixed tree; its barriers stand between the reads above and the writes below

    const float y0 = eps / (float)N, coef = wi * c / W;
    float sp = 0.f, sv = 0.f;
    auto seed = [&](float v) {
        const float e = expf(-fabsf(v));  // in (0, 1]: softplus and sigmoid stay finite for any finite score
        sp += fmaxf(v, 0.f) + log1pf(e);
        sv += v;
        return coef * ((v >= 0.f ? 1.f : e) / (1.f + e) - y0);
    };
    int64_t j = tid;
    for (; j + 768 < N; j += 1024) {  // four strides' loads in flight at a time (a plain loop is one round trip per column)
        float v[4];
#pragma unroll
        for (int z = 0; z < 4; ++z) v[z] = row[j + 256 * z];
#pragma unroll
        for (int z = 0; z < 4; ++z) row[j + 256 * z] = seed(v[z]);
    }
    for (; j < N; j += 256) row[j] = seed(row[j]);
    for (int64_t p = N + tid; p < ld; p += 256) row[p] = 0.f;  // the forward's pad columns
    sp = block_sum_256(sp, red);
    sv = block_sum_256(sv, red);  // (the dense pass is behind these barriers)
    const float off = coef * (1.f - eps);
    for (int64_t k = lo + tid; k < hi; k += 256) row[table_row(keys[k] - base, N)] -= off;
    if (tid == 0) {
        pos[i] = p_i;
        rowpart[i] = wi * c * (sp - y0 * sv - (1.f - eps) * lab);
    }
}

void all_bce_launch(float *S, int64_t B, int64_t N, int64_t ld, const int64_t *sample, bool head, int64_t R, const int64_t *keys,
                           int64_t n_keys, const float *weight, const float *weight_sum, float eps, bool sum_over_entities, float *loss,
                           float *pos, float *scratch, hipStream_t st) {
    all_loss_launch(weight, weight_sum, B, loss, scratch, st, [&](const RowLoss &L) {
        hipLaunchKernelGGL(all_bce_kernel, dim3((unsigned)B), dim3(256), 0, st, S, (int)B, N, ld, sample, head ? 1 : 0, R, keys, n_keys,
                           weight, L.scal_in, L.scal_out, eps, sum_over_entities ? 1.f : 1.f / (float)N, pos, L.rowpart);
    });
}

// ---- filtered 1vsAll (include/mkb_hip.h, "filtered 1vsAll"): the softmax over the row WITHOUT the query's other known answers,
//     C_i = [0, N) \ (A_i \ {t_i}),  n_i = |C_i|,  y_ij = (1 - eps) [j = t_i] + eps / n_i,
//     row_i = log sum_{C_i} exp(s_ij / T) - (1 - eps) s_it / T - (eps / n_i) sum_{C_i} s_ij / T,  dS_ij = (w_i / (W T)) (p_ij - y_ij) on C_i, 0 off it
// A_i: the key range of all_bce_kernel.  One 256-lane workgroup per row.  The filtered columns are marked first, in S itself (it is
// overwritten anyway; keys are unique and the target is never marked: one writer per element, and the target's score stays
// readable): -inf, which no maximum picks, whose exponent is 0 and which the linear sum skips by test -- nothing is added and taken
// back.  Then all_softmax_kernel's three passes, LDS staging up to kAllStageCols, the global loads four strides at a time.  The sums
// are taken relative to the row maximum m (the weights of m in the row add up to 1 - (1 - eps) - n_i eps / n_i = 0):
//     row_i = log Z - (1 - eps) (s_it - m) / T - (eps / n_i) sum_{C_i} (s_ij - m) / T,   Z = sum_{C_i} exp((s_ij - m) / T) >= 1.
// scal / scal_out / rowpart: as for all_softmax_kernel.

// f(j, row[j]) for the lane's columns j = tid, tid + 256, ... < N in that order, four strides' loads in flight at a time (f may
// write row[j]: a lane only ever touches its own columns)
template <class F>
__device__ __forceinline__ void row_cols_256(float *__restrict__ row, int64_t N, F &&f) {
    int64_t j = threadIdx.x;
    for (; j + 768 < N; j += 1024) {
        float v[4];
#pragma unroll
        for (int z = 0; z < 4; ++z) v[z] = row[j + 256 * z];
#pragma unroll
        for (int z = 0; z < 4; ++z) f(j + 256 * z, v[z]);
    }
    for (; j < N; j += 256) f(j, row[j]);
}

__global__ __launch_bounds__(256) void all_softmax_filtered_kernel(float *__restrict__ S, int B, int64_t N, int64_t ld,
                                                                   const int64_t *__restrict__ target, int64_t tstride,
                                                                   const int64_t *__restrict__ sample, int head, int64_t R,
                                                                   const int64_t *__restrict__ keys, int64_t n_keys,
                                                                   const float *__restrict__ w, const float *__restrict__ scal,
                                                                   float *__restrict__ scal_out, float inv_T, float eps,
                                                                   float *__restrict__ pos, float *__restrict__ rowpart) {
    __shared__ float red[4];
    extern __shared__ float s_row[];
    const int tid = threadIdx.x;
    const int64_t i = blockIdx.x;
    float *row = S + i * ld;
    const bool staged = N <= kAllStageCols;
    const int64_t *s = sample + 3 * i;
    // (an id outside its table counts as the nearest row, so that no marked column leaves the row: the glue flags it, mkb_check_ids)
    const int64_t q = table_row(s[head ? 2 : 0], N) * R + table_row(s[1], R), base = q * N;
    const int64_t t = table_row(target[i * tstride], N);
    const int64_t lo = lower_bound_dev(keys, n_keys, base), hi = lower_bound_dev(keys, n_keys, base + N);  // (uniform; empty: lo == hi)
    const float p_i = row[t];  // before anything is overwritten (and column t is never marked)
    const float wi = w ? w[i] : 1.f;

    int own = 0;  // the target is one of the keys: it stays in the row
    for (int64_t k = lo + tid; k < hi; k += 256) {
        const int64_t c = table_row(keys[k] - base, N);
        if (c == t) own = 1;
        else row[c] = -INFINITY;
    }
    own = __syncthreads_or(own);  // (its barrier stands between the marks and the passes that read them)
    const int64_t n = N - (hi - lo) + (own ? 1 : 0);  // >= 1: the target
    const float W = row_loss_weight_sum(scal, scal_out, w, B, red);

    float m = -INFINITY;
    row_cols_256(row, N, [&](int64_t j, float v) {
        m = fmaxf(m, v);
        if (staged) s_row[j] = v;
    });
    m = block_max_256(m, red);  // finite: the target's score is in it

    // every exponent and every term of the linear sum relative to the row maximum; a marked column: exponent 0, no linear term
    float z = 0.f, sv = 0.f;
    auto term = [&](float v) {
        const float d = (v - m) * inv_T;
        if (v != -INFINITY) sv += d;
        const float e = expf(d);
        z += e;
        return v != -INFINITY ? e : -1.f;  // (staged: the mark outlives the exponent, which may be 0 for a kept column too)
    };
    if (staged)
        for (int64_t j = tid; j < N; j += 256) s_row[j] = term(s_row[j]);
    else
        row_cols_256(row, N, [&](int64_t, float v) { term(v); });
    z = block_sum_256(z, red);  // lane-strided partial sums, then the fixed tree
    sv = block_sum_256(sv, red);
    const float inv = 1.f / z, coef = wi * inv_T / W;
    const float y0 = eps / (float)n, yt = 1.f - eps * ((float)(n - 1) / (float)n);  // (n = 1: the target's label is exactly 1)
    auto seed = [&](int64_t j, float e) { return e < 0.f ? 0.f : coef * (e * inv - (j == t ? yt : y0)); };
    if (staged)
        for (int64_t j = tid; j < N; j += 256) row[j] = seed(j, s_row[j]);
    else
        row_cols_256(row, N, [&](int64_t j, float v) { row[j] = seed(j, v != -INFINITY ? expf((v - m) * inv_T) : -1.f); });
    for (int64_t j = N + tid; j < ld; j += 256) row[j] = 0.f;  // the forward's pad columns
    if (tid == 0) {
        pos[i] = p_i;
        rowpart[i] = wi * (logf(z) - (1.f - eps) * ((p_i - m) * inv_T) - y0 * sv);
    }
}

void all_softmax_filtered_launch(float *S, int64_t B, int64_t N, int64_t ld, const int64_t *target, int64_t tstride,
                                        const int64_t *sample, bool head, int64_t R, const int64_t *keys, int64_t n_keys,
                                        const float *weight, const float *weight_sum, float T, float eps, float *loss, float *pos,
                                        float *scratch, hipStream_t st) {
    all_loss_launch(weight, weight_sum, B, loss, scratch, st, [&](const RowLoss &L) {
        const size_t lds = N <= kAllStageCols ? (size_t)N * sizeof(float) : 0;
        hipLaunchKernelGGL(all_softmax_filtered_kernel, dim3((unsigned)B), dim3(256), lds, st, S, (int)B, N, ld, target, tstride, sample,
                           head ? 1 : 0, R, keys, n_keys, weight, L.scal_in, L.scal_out, 1.f / T, eps, pos, L.rowpart);
    });
}

int softmax_check(const void *S, int64_t B, int64_t N, int64_t ld, const void *target, int64_t tstride, float T, const void *loss,
                         const void *pos, const void *scratch) {
    MKB_REQUIRE(S && target && loss && pos && scratch, "null pointer");
    MKB_REQUIRE(T - T == 0.f && T > 0.f, "the softmax temperature must be finite and > 0");
    MKB_REQUIRE(B >= 1, "B must be >= 1");
    MKB_REQUIRE(N >= 1 && ld >= N && tstride >= 1, "need N >= 1, ld >= N and target_stride >= 1");
    MKB_REQUIRE(B <= INT32_MAX && ld <= INT32_MAX && B * ld <= INT32_MAX, "B * ld must stay below 2^31");
    return MKB_OK;
}

// what the entry points that read the key arrays (KvsAll, filtered 1vsAll: `what`) check of their label arguments (N, R: the table
// sizes the keys were built for)
int bce_check(int64_t N, int64_t R, int mode, const void *keys, int64_t n_keys, float eps, const char *what) {
    MKB_REQUIRE(mode == MKB_MODE_HEAD || mode == MKB_MODE_TAIL, "%s needs head-batch or tail-batch", what);
    MKB_REQUIRE(n_keys >= 0 && (keys || n_keys == 0), "keys may be null only with n_keys == 0, and n_keys must be >= 0");
    MKB_REQUIRE(eps - eps == 0.f && eps >= 0.f && eps < 1.f, "the label smoothing must be finite and in [0, 1)");
    int64_t nq, top;  // the largest value a range bound takes: ((N - 1) R + R - 1) N + N <= (N R + R) N
    MKB_REQUIRE(N >= 1 && R >= 1 && !__builtin_mul_overflow(N, R, &nq) && !__builtin_add_overflow(nq, R, &nq) &&
                    !__builtin_mul_overflow(nq, N, &top),
                "(n_entity * n_relation + n_relation) * n_entity must fit a signed 64-bit key");
    return MKB_OK;
}

// ---- the family of the two models whose all-entity block is one product, for the protocol of all_host.h
struct DotFamily {
    static constexpr bool covers(int model) { return model == MKB_COMPLEX || model == MKB_DISTMULT; }
    static constexpr const char *refusal =
        "1vsAll covers ComplEx and DistMult, whose all-entity block is one matrix product; for TransE, RotatE and "
        "pRotatE use the sampled softmax (losses.CrossEntropy), or the all-entity calls of the distance models, "
        "mkb_dist_all_* (fused.DistanceAllStep)";
    static constexpr const char *mode_text = "1vsAll needs head-batch or tail-batch";
    struct Launch {};  // (the two backward products are planned where they are launched: plan_gemm)

    // the partial buffer of the two backward products, used one after the other; nothing behind the loss scratch
    static FamilyBytes plan(const mkb_tables_t *tb, int64_t B, Launch &) {
        const int64_t N = tb->n_entity, Npad = all_npad(N), De = tb->entity_dim;
        const GemmSwitches sw{false, false, true};  // (part_bound does not depend on the switches)
        const size_t part = std::max(plan_gemm(all_dq_shape(B, N, De, Npad, true, true), all_dq_limits(), sw).part_bound,
                                     plan_gemm(all_de_shape(B, N, De, Npad, true), all_de_limits(N, De), sw).part_bound);
        return FamilyBytes{part * 4, 0};
    }

    // (never reached: the two models' blocks are finished scores on every route of run_rank, c0 = 0, c1 = 1)
    static void finish_block(float *, int64_t, int64_t, int64_t, float, float, hipStream_t) {}

    // dS [B, ld] -> g_ent, g_rel (accumulated)
    template <int MODEL, bool HEAD>
    static int bwd(const mkb_tables_t *tb, const mkb_grads_t *gr, const int64_t *sample, int64_t B, const float *dS, int64_t ld,
                   bool gathered, const AllPlan<DotFamily> &P, const AllWs &w, hipStream_t st) {
        const int64_t N = tb->n_entity, De = tb->entity_dim;
        const GemmSwitches sw = gemm_switches_from_env();
        const bool al = (((uintptr_t)dS | (uintptr_t)tb->ent | (uintptr_t)gr->g_ent) & 15) == 0;  // (Q, dQ: the 256-byte aligned workspace)
        ChainArgs A;
        if (int rc = all_chain_open<HEAD>(tb, gr, sample, B, w.dQ, w.stash, w.sort, P.sort, st, A)) return rc;
        {
            const GemmPlan plan = plan_gemm(all_dq_shape(B, N, De, ld, gathered, al), all_dq_limits(), sw);
            GemmArgs G = gemm_args(plan);
            G.A = dS; G.B = tb->ent; G.C = w.dQ; G.b_idx = gathered ? w.ids : nullptr;
            if (int rc = launch_gemm<true, false, GEMM_STORE>(plan, G, st, w.part)) return rc;
        }
        {
            const GemmPlan plan = plan_gemm(all_de_shape(B, N, De, ld, al), all_de_limits(N, De), sw);
            GemmArgs G = gemm_args(plan);
            G.A = dS; G.B = w.Q; G.C = gr->g_ent;
            if (int rc = launch_gemm<false, false, GEMM_ACCUM>(plan, G, st, w.part)) return rc;
        }
        hipLaunchKernelGGL((all_chain_kernel<MODEL, HEAD>), dim3((unsigned)(2 * B)), dim3(256), 0, st, A);
        MKB_LAUNCH_CHECK();
        return MKB_OK;
    }
};

}  // namespace mkb

using namespace mkb;

// (the calls that take tables: the bodies of all_host.h for DotFamily)
extern "C" int64_t mkb_all_step_workspace_bytes(const mkb_tables_t *tb, int64_t B) { return all_workspace_bytes<DotFamily>(tb, B); }

extern "C" int mkb_all_score_fwd(const mkb_tables_t *tb, const int64_t *sample, int64_t B, int mode, float *scores, void *ws,
                                 int64_t ws_bytes, void *stream) {
    return all_score_fwd<DotFamily>(tb, sample, B, mode, scores, ws, ws_bytes, stream);
}

extern "C" int mkb_all_softmax(float *S, int64_t B, int64_t N, int64_t ld, const int64_t *target, int64_t target_stride,
                               const float *weight, const float *weight_sum, float T, float *loss, float *pos, float *scratch,
                               void *stream) {
    if (int rc = softmax_check(S, B, N, ld, target, target_stride, T, loss, pos, scratch)) return rc;
    all_softmax_launch(S, B, N, ld, target, target_stride, weight, weight_sum, T, loss, pos, scratch, (hipStream_t)stream);
    MKB_LAUNCH_CHECK();
    return MKB_OK;
}

extern "C" int mkb_all_score_bwd(const mkb_tables_t *tb, const mkb_grads_t *gr, const int64_t *sample, int64_t B, int mode,
                                 const float *dscore, int64_t ld, void *ws, int64_t ws_bytes, void *stream) {
    return all_score_bwd<DotFamily>(tb, gr, sample, B, mode, dscore, ld, ws, ws_bytes, stream);
}

extern "C" int mkb_all_step(const mkb_tables_t *tb, const mkb_grads_t *gr, const int64_t *sample, const float *weight, int64_t B,
                            int mode, float temperature, const float *weight_sum, float *loss, float *pos, void *ws, int64_t ws_bytes,
                            void *stream) {
    return all_softmax_step<DotFamily>(tb, gr, sample, weight, B, mode, temperature, weight_sum, loss, pos, ws, ws_bytes, stream);
}

extern "C" int mkb_all_bce(float *S, int64_t B, int64_t N, int64_t ld, const int64_t *sample, int mode, int64_t n_relation,
                           const int64_t *keys, int64_t n_keys, const float *weight, const float *weight_sum, float smoothing,
                           int sum_over_entities, float *loss, float *pos, float *scratch, void *stream) {
    if (int rc = softmax_check(S, B, N, ld, sample, 1, 1.f, loss, pos, scratch)) return rc;
    if (int rc = bce_check(N, n_relation, mode, keys, n_keys, smoothing)) return rc;
    all_bce_launch(S, B, N, ld, sample, mode == MKB_MODE_HEAD, n_relation, keys, n_keys, weight, weight_sum, smoothing,
                   sum_over_entities != 0, loss, pos, scratch, (hipStream_t)stream);
    MKB_LAUNCH_CHECK();
    return MKB_OK;
}

extern "C" int mkb_all_kvs_step(const mkb_tables_t *tb, const mkb_grads_t *gr, const int64_t *sample, const float *weight, int64_t B,
                                int mode, const int64_t *keys, int64_t n_keys, float smoothing, int sum_over_entities,
                                const float *weight_sum, float *loss, float *pos, void *ws, int64_t ws_bytes, void *stream) {
    return all_kvs_step<DotFamily>(tb, gr, sample, weight, B, mode, keys, n_keys, smoothing, sum_over_entities, weight_sum, loss, pos, ws,
                                   ws_bytes, stream);
}

extern "C" int mkb_all_softmax_filtered(float *S, int64_t B, int64_t N, int64_t ld, const int64_t *target, int64_t target_stride,
                                        const int64_t *sample, int mode, int64_t n_relation, const int64_t *keys, int64_t n_keys,
                                        const float *weight, const float *weight_sum, float T, float smoothing, float *loss, float *pos,
                                        float *scratch, void *stream) {
    MKB_REQUIRE(sample, "null pointer");
    if (int rc = softmax_check(S, B, N, ld, target, target_stride, T, loss, pos, scratch)) return rc;
    if (int rc = bce_check(N, n_relation, mode, keys, n_keys, smoothing, "filtered 1vsAll")) return rc;
    all_softmax_filtered_launch(S, B, N, ld, target, target_stride, sample, mode == MKB_MODE_HEAD, n_relation, keys, n_keys, weight,
                                weight_sum, T, smoothing, loss, pos, scratch, (hipStream_t)stream);
    MKB_LAUNCH_CHECK();
    return MKB_OK;
}

extern "C" int mkb_all_filtered_step(const mkb_tables_t *tb, const mkb_grads_t *gr, const int64_t *sample, const float *weight, int64_t B,
                                     int mode, const int64_t *keys, int64_t n_keys, float T, float smoothing, const float *weight_sum,
                                     float *loss, float *pos, void *ws, int64_t ws_bytes, void *stream) {
    return all_filtered_step<DotFamily>(tb, gr, sample, weight, B, mode, keys, n_keys, T, smoothing, weight_sum, loss, pos, ws, ws_bytes,
                                        stream);
}
