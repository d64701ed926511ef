// mkb_rank: filtered link-prediction rank of each test triple's target among ALL entities, on the device.
//
// Replaces evaluation.Evaluation.compute_score for head-/tail-batch (evaluation/evaluation.py:217-279) together
// with the candidate list / filter bias that datasets.base.TestDataset builds per item on the host
// (datasets/base.py:196-241): candidates are the n_entity ids in order; a candidate whose corrupted triple is
// ANOTHER true triple gets bias -100000 (i.e. can never outrank the target); rank = 1 + number of candidates
// scoring above the target (the reference reads it off a descending argsort, evaluation.py:245-262).
//
// Kernel 1  all_fwd : scores of B queries against every entity row.  Same lane-owns-dims tiling as the pooled
//           forward (8 rows per 1024-lane workgroup, swap/DPP wave reduction, LDS cross-wave combine per 16
//           candidates) but the candidates are simply consecutive table rows, split into slices over grid.y.
//           RotatE / TransE: the pooled forward's outer-product register tile instead; ComplEx / DistMult: one matrix-core
//           product (run_rank), planned by plan_gemm (gemm_plan.h) with this route's limits -- no partial buffer, no K split --
//           and the three MKB_GEMM_* switches, which run_rank reads there, once per call.
// Kernel 2  rank    : one wave per query: count scores above the target's, then walk the query's true set
//           (a contiguous range of the sorted key array) and take back the ones that were counted.
#include "common.h"
#include "rank_all.h"    // Kernel 1 and run_rank, the all-entity block on its three routes (shared with score_all.hip)
#include "rank_order.h"  // ranks_before: the order every rank and top k here is counted in

#include <algorithm>

namespace mkb {

// one wave per query
// (c0, c1): S holds finished scores (0, 1) or the raw pair sums of the register-tile route, finished here as c0 + c1 * sum -- the
// same fp32 operation the all-entity kernel applies, so that ties fall as they do there
__global__ __launch_bounds__(256) void rank_kernel(const float *__restrict__ S, const int64_t *__restrict__ sample, int B,
                                                   int64_t N, int64_t R, int head_mode,
                                                   const int64_t *__restrict__ keys, int64_t nk,
                                                   int64_t *__restrict__ rank, float c0, float c1, int64_t ld) {  // ld: floats between rows of S
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= B) return;
    const int64_t h = sample[3 * (int64_t)i], r = sample[3 * (int64_t)i + 1], t = sample[3 * (int64_t)i + 2];
    const int64_t target = head_mode ? h : t;
    const float *row = S + (int64_t)i * ld;
    auto val = [&](int64_t e) { return c0 + c1 * row[e]; };
    const float st = val(target);
    int64_t cnt = 0;
    // eight strides' loads at a time (a loop with a run-time trip count waits for every load before it issues the next: 227 round
    // trips per query at FB15k-237's size)
    for (int64_t e0 = lane; e0 < N; e0 += 64 * 8) {
        float v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = row[min(e0 + 64 * k, N - 1)];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int64_t e = e0 + 64 * k;
            cnt += (e < N && ranks_before(c0 + c1 * v[k], e, st, target)) ? 1 : 0;
        }
    }
    // other true triples (base.py:213-216 / 229-232): take back those that were counted
    const int64_t base = ((head_mode ? t : h) * R + r) * N;  // keys of this (fixed entity, relation) pair are contiguous
    int64_t lo = 0, hi = nk;
    while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (keys[mid] < base) lo = mid + 1; else hi = mid; }
    for (int64_t k = lo + lane; k < nk; k += 64) {
        const int64_t key = keys[k];
        if (key >= base + N) break;
        const int64_t e = key - base;
        if (e != target && ranks_before(val(e), e, st, target)) cnt -= 1;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off, 64);
    if (lane == 0) rank[i] = cnt + 1;
}


// ---- filtered top k (mkb_topk) ----------------------------------------------------------------------------------------------------
// One workgroup per query selects the k best entries of its row of S by the order of ranks_before (NaN first, then higher score,
// then lower entity id), leaving out the query's true set (the contiguous range of the sorted key array rank_kernel walks; with
// MKB_TOPK_KEEP_TARGET the target stays in).  The order is that of a composite 64-bit key: the order-preserving 32-bit image of the
// finished score (NaN on top, -0 folded onto +0 so that the two tie as they compare) in the high word, ~id in the low word.
//   1. radix select of the k-th largest 32-bit image, 11 + 11 + 10 bits: three passes over the row, each an LDS histogram of the
//      entries that match the prefix found so far; the filtered entries are then walked (their key range) and taken back out of
//      the counts, so the filtered set may be any size.  Ends with the threshold image T and `need`, the number of entries at T
//      that belong to the top k (all of them when the row has fewer than k candidates left: T = 0, below every image).
//   2. gather: one more pass appends every unfiltered entry above T and at T to an LDS buffer (a binary search of the key range
//      per appended entry).  More than kTopkCap entries tie at T only for a collapsed row: those are then taken in id order, the
//      first `need` of them.
//   3. bitonic sort of the buffer (at most kTopkCap composite keys, descending) in LDS; the first k are written out with their
//      scores re-read from S and finished as rank_kernel / export_scores_kernel finish them (bit-identical).  Slots past the
//      candidates left: id -1, score -inf.
// Three instantiations of the one kernel:
//   kTopkPlain  -- mkb_topk;
//   kTopkMasked -- mkb_topk_masked: only the entities whose bit is set in cand_bits [ceil(N / 32)] are candidates.  An entity outside
//                  the mask is treated as a filtered one at every step (not counted in the histograms, not taken back out of them,
//                  not gathered, not taken by the collapsed-row fallback), MKB_TOPK_KEEP_TARGET included.  The mask is read from
//                  global memory, not staged in LDS: it is 1/32 of the bytes of the score row it sits next to, every workgroup reads
//                  the same words (they stay in L2 after the first few rows), and the eight mask loads of a strided step are issued
//                  with the eight score loads; staging it would need an LDS block sized by N (15 KB at YAGO3-10's 123 k entities,
//                  on top of the kernel's 25 KB) and cost occupancy on every shape;
//   kTopkBlock  -- mkb_topk_block: a caller's fp32 block [B, N] with row stride ld: no sample, no true keys, no finisher (the
//                  scores handed out are the block's own values, bit for bit).
// and a fourth, kTopkNearest (mkb_topk_nearest): kTopkBlock on a block of squared L2 distances, selected on -d (the k SMALLEST
// distances; NaN first, ties to the lower column as before); out go the candidate ids cand[column] and the distances themselves,
// padded with -1 / +inf.
constexpr int kTopkThreads = 256, kTopkCap = 2048;
constexpr int kTopkPlain = 0, kTopkMasked = 1, kTopkBlock = 2, kTopkNearest = 3;

__device__ __forceinline__ uint32_t order_image(float f) {
    if (f != f) return 0xFFFFFFFFu;
    const uint32_t b = f == 0.f ? 0u : __float_as_uint(f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

struct TopkArgs {
    const float *S;
    const int64_t *sample, *keys;
    int64_t *ids;
    float *scores;
    int64_t B, N, R, nk, ld;
    int head_mode, k, keep_target;
    float c0, c1;
};
// kTopkMasked's arguments: the candidate bitmask, bit e % 32 of word e / 32 (a struct of its own, so that kTopkPlain's kernel
// arguments keep their layout)
struct TopkMaskedArgs : TopkArgs {
    const uint32_t *cand;
};
// kTopkNearest's arguments: the candidate ids [N] of the block's columns
struct TopkNearestArgs : TopkArgs {
    const int64_t *cand;
};

// (static: with internal linkage the kTopkPlain instantiation compiles to the very code and LDS layout of the non-template kernel
// mkb_topk launched before the two other instantiations were added)
template <int VAR, class Args = TopkArgs>
static __global__ __launch_bounds__(kTopkThreads) void topk_kernel(Args A) {
    constexpr bool MASKED = VAR == kTopkMasked, NEAREST = VAR == kTopkNearest, BLOCK = VAR == kTopkBlock || NEAREST;
    __shared__ uint32_t s_hist[2048];
    __shared__ uint32_t s_scan[kTopkThreads];
    __shared__ uint64_t s_buf[kTopkCap];
    __shared__ int64_t s_range[2];
    __shared__ uint32_t s_sel[2], s_cnt;
    constexpr int T = kTopkThreads;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t N = A.N;
    for (int64_t i = blockIdx.x; i < A.B; i += gridDim.x) {
        // (kTopkBlock: no sample, no keys -- keep = -1, base = 0 and an empty key range, so nothing is filtered)
        const int64_t h = BLOCK ? 0 : A.sample[3 * i], r = BLOCK ? 0 : A.sample[3 * i + 1], t = BLOCK ? 0 : A.sample[3 * i + 2];
        const int64_t keep = A.keep_target ? (A.head_mode ? h : t) : -1;
        const int64_t base = ((A.head_mode ? t : h) * A.R + r) * N;  // as in rank_kernel
        const float *row = A.S + i * A.ld;
        if (tid < 2) {
            const int64_t want = tid == 0 ? base : base + N;
            int64_t lo = 0, hi = A.nk;
            while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (A.keys[mid] < want) lo = mid + 1; else hi = mid; }
            s_range[tid] = lo;
        }
        __syncthreads();
        const int64_t klo = s_range[0], khi = s_range[1];
        auto fin = [&](float x) {
            if constexpr (NEAREST) return -x;
            else if constexpr (BLOCK) return x;
            else return A.c0 + A.c1 * x;
        };
        auto image = [&](int64_t e) { return order_image(fin(row[e])); };
        auto cand_word = [&](int64_t e) -> uint32_t {
            if constexpr (MASKED) return A.cand[e >> 5];
            else return 1u;
        };
        auto in_word = [&](uint32_t w, int64_t e) {
            if constexpr (MASKED) return ((w >> (e & 31)) & 1u) != 0u;
            else return true;
        };
        auto is_cand = [&](int64_t e) { return in_word(cand_word(e), e); };
        auto filtered = [&](int64_t e) {
            if (e == keep) return false;
            int64_t lo = klo, hi = khi;
            while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (A.keys[mid] < base + e) lo = mid + 1; else hi = mid; }
            return lo < khi && A.keys[lo] == base + e;
        };

        // 1. radix select
        uint32_t prefix = 0, mask = 0, need = (uint32_t)A.k;
        bool all = false;
        for (int p = 0; p < 3; ++p) {
            const int shift = p == 0 ? 21 : p == 1 ? 10 : 0;
            const uint32_t bins = p == 2 ? 1024u : 2048u;
            for (int b = tid; b < 2048; b += T) s_hist[b] = 0;
            __syncthreads();
            for (int64_t e0 = tid; e0 < N; e0 += T * 8) {  // eight strides' loads in flight (see rank_kernel)
                float v[8];
                uint32_t w[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) v[j] = row[min(e0 + T * j, N - 1)];
#pragma unroll
                for (int j = 0; j < 8; ++j) w[j] = cand_word(min(e0 + T * j, N - 1));
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const uint32_t u = order_image(fin(v[j]));
                    if (e0 + T * j < N && (u & mask) == prefix && in_word(w[j], e0 + T * j)) atomicAdd(&s_hist[(u >> shift) & (bins - 1)], 1u);
                }
            }
            __syncthreads();  // (an entry counted above and taken back below may otherwise meet in the other order: unsigned wrap is harmless, but keep it plain)
            for (int64_t q = klo + tid; q < khi; q += T) {
                const int64_t e = A.keys[q] - base;
                if (e == keep) continue;
                const uint32_t u = image(e);
                if ((u & mask) == prefix && is_cand(e)) atomicSub(&s_hist[(u >> shift) & (bins - 1)], 1u);
            }
            __syncthreads();
            // thread tid owns bins [8 tid, 8 tid + 8): inclusive suffix sums over the threads
            uint32_t own = 0;
#pragma unroll
            for (int j = 0; j < 8; ++j) own += s_hist[8 * tid + j];
            s_scan[tid] = own;
            __syncthreads();
            for (int off = 1; off < T; off <<= 1) {
                const uint32_t x = tid + off < T ? s_scan[tid + off] : 0u;
                __syncthreads();
                s_scan[tid] += x;
                __syncthreads();
            }
            const uint32_t incl = s_scan[tid], total = s_scan[0];
            if (total < need) {  // (pass 0 only) fewer than k candidates left: take them all
                all = true;
                break;
            }
            uint32_t above = incl - own;
            if (above < need && need <= incl) {
                for (int j = 7; j >= 0; --j) {
                    const uint32_t c = s_hist[8 * tid + j];
                    if (above + c >= need) { s_sel[0] = 8 * tid + j; s_sel[1] = need - above; break; }
                    above += c;
                }
            }
            __syncthreads();
            prefix |= s_sel[0] << shift;
            mask |= (bins - 1) << shift;
            need = s_sel[1];
            __syncthreads();
        }
        const uint32_t thr = all ? 0u : prefix;

        // 2. gather
        if (tid == 0) s_cnt = 0;
        __syncthreads();
        for (int64_t e0 = tid; e0 < N; e0 += T * 8) {
            float v[8];
            uint32_t w[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = row[min(e0 + T * j, N - 1)];
#pragma unroll
            for (int j = 0; j < 8; ++j) w[j] = cand_word(min(e0 + T * j, N - 1));
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int64_t e = e0 + T * j;
                const uint32_t u = order_image(fin(v[j]));
                if (e < N && u >= thr && in_word(w[j], e) && !filtered(e)) {
                    const uint32_t slot = atomicAdd(&s_cnt, 1u);
                    if (slot < (uint32_t)kTopkCap) s_buf[slot] = ((uint64_t)u << 32) | (uint32_t)~(uint32_t)e;
                }
            }
        }
        __syncthreads();
        uint32_t n = s_cnt;
        if (n > (uint32_t)kTopkCap) {  // uniform: more than kTopkCap - (k - need) entries tie at T (a collapsed row)
            __syncthreads();
            if (tid == 0) s_cnt = 0;
            __syncthreads();
            for (int64_t e = tid; e < N; e += T) {  // the k - need < k entries above T
                const uint32_t u = image(e);
                if (u > thr && is_cand(e) && !filtered(e)) {
                    const uint32_t slot = atomicAdd(&s_cnt, 1u);
                    if (slot < (uint32_t)A.k) s_buf[slot] = ((uint64_t)u << 32) | (uint32_t)~(uint32_t)e;  // (< k by the select)
                }
            }
            __syncthreads();
            const uint32_t at = min(s_cnt, (uint32_t)A.k);
            uint32_t taken = 0;
            for (int64_t e0 = 0; e0 < N && taken < need; e0 += T) {  // ... and the first `need` ties in id order
                const int64_t e = e0 + tid;
                const bool tie = e < N && image(e) == thr && is_cand(e) && !filtered(e);
                const uint64_t m = __ballot(tie);
                __syncthreads();
                if (lane == 0) s_scan[wave] = (uint32_t)__popcll(m);
                __syncthreads();
                uint32_t before = 0, here = 0;
                for (int w = 0; w < T / 64; ++w) {
                    before += w < wave ? s_scan[w] : 0u;
                    here += s_scan[w];
                }
                const uint32_t pos = taken + before + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
                if (tie && pos < need && at + pos < (uint32_t)kTopkCap) s_buf[at + pos] = ((uint64_t)thr << 32) | (uint32_t)~(uint32_t)e;
                taken += here;
            }
            n = min(at + min(need, taken), (uint32_t)kTopkCap);
            __syncthreads();
        }

        // 3. bitonic sort, descending, of the n <= kTopkCap keys (padded with 0, below every key)
        uint32_t P = 2;
        while (P < n) P <<= 1;
        for (uint32_t j = n + tid; j < P; j += T) s_buf[j] = 0;
        __syncthreads();
        for (uint32_t size = 2; size <= P; size <<= 1)
            for (uint32_t stride = size >> 1; stride > 0; stride >>= 1) {
                for (uint32_t q = tid; q < P / 2; q += T) {
                    const uint32_t a = 2 * q - (q & (stride - 1)), b = a + stride;
                    const uint64_t x = s_buf[a], y = s_buf[b];
                    if ((x < y) == ((a & size) == 0)) { s_buf[a] = y; s_buf[b] = x; }
                }
                __syncthreads();
            }
        for (int j = tid; j < A.k; j += T) {
            const int64_t o = i * A.k + j;
            if ((uint32_t)j < n) {
                const int64_t e = (int64_t)(uint32_t)~(uint32_t)s_buf[j];
                if constexpr (NEAREST) {
                    A.ids[o] = A.cand[e];
                    A.scores[o] = row[e];
                } else {
                    A.ids[o] = e;
                    A.scores[o] = fin(row[e]);
                }
            } else {
                A.ids[o] = -1;
                A.scores[o] = NEAREST ? INFINITY : -INFINITY;
            }
        }
        __syncthreads();
    }
}

// ---- exact squared-L2 k nearest rows (mkb_topk_nearest) ------------------------------------------------------------------------
// S[i, c] = sum_j (Q[i, j] - X[cand[c], j])^2 on the general route (any D, any row strides, any alignment): one lane per candidate,
// the queries loop over grid.y.  The even elements and the odd ones are summed in two fma chains and added at the end, the order of
// the register tile's kTileL2 accumulators (score_pool_tile.h), so that both routes give the same bits.  Not a hot path: the
// product's rows take the tile (D % 4 == 0, D >= 64, contiguous rows).
__global__ __launch_bounds__(256) void l2_block_kernel(const float *__restrict__ Q, int64_t ldq, const float *__restrict__ X, int64_t ldx,
                                                       const int64_t *__restrict__ cand, int64_t n_cand, int64_t B, int64_t D,
                                                       float *__restrict__ S) {
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= n_cand) return;
    const float *x = X + cand[c] * ldx;
    for (int64_t i = blockIdx.y; i < B; i += gridDim.y) {
        const float *q = Q + i * ldq;
        float ev = 0.f, od = 0.f;
        int64_t j = 0;
        for (; j + 1 < D; j += 2) {
            const float a = q[j] - x[j], b = q[j + 1] - x[j + 1];
            ev = fmaf(a, a, ev);
            od = fmaf(b, b, od);
        }
        if (j < D) {
            const float a = q[j] - x[j];
            ev = fmaf(a, a, ev);
        }
        S[i * n_cand + c] = ev + od;
    }
}


}  // namespace mkb

using namespace mkb;

extern "C" int64_t mkb_rank_workspace_bytes(const mkb_tables_t *tb, int64_t B) {
    if (!tb || B <= 0) return 0;
    return (int64_t)(((size_t)B * tb->entity_dim * 4 + 255) & ~(size_t)255) + (int64_t)(((size_t)B * (tb->n_entity + 3) * 4 + 255) & ~(size_t)255) +
           (int64_t)(tb->n_entity + 3) * 8;
}

// workspace carve-up shared by mkb_rank and mkb_topk: Q [B, De], S [B, N (+3)], the id list [N + 3]
struct RankWs {
    float *Q, *S;
    int64_t *ids;
};
static RankWs carve_ws(const mkb_tables_t *tb, int64_t B, void *ws) {
    RankWs w;
    w.Q = (float *)ws;
    w.S = (float *)((unsigned char *)ws + (((size_t)B * tb->entity_dim * 4 + 255) & ~(size_t)255));
    w.ids = (int64_t *)((unsigned char *)w.S + (((size_t)B * (tb->n_entity + 3) * 4 + 255) & ~(size_t)255));  // [N + 3] 0, 1, ... (tile / GEMM routes)
    return w;
}

static int rank_impl(const mkb_tables_t *tb, const int64_t *sample, int64_t B, int mode, const int64_t *true_keys,
                     int64_t n_true, int64_t *rank, float *scores, void *ws, int64_t ws_bytes, void *stream) {
    if (int rc = validate_tables(tb)) return rc;
    MKB_REQUIRE(sample && rank && ws && (true_keys || n_true == 0), "null pointer");
    MKB_REQUIRE(mode == MKB_MODE_HEAD || mode == MKB_MODE_TAIL, "mkb_rank needs head-batch or tail-batch");
    MKB_REQUIRE(B > 0 && B <= INT32_MAX, "bad B");
    MKB_REQUIRE(ws_bytes >= mkb_rank_workspace_bytes(tb, B) && (((uintptr_t)ws) & 255) == 0, "workspace too small / unaligned");
    const int NU = tb->model == MKB_ROTATE ? tb->hidden_dim : (int)tb->entity_dim;
    MKB_REQUIRE(NU <= 4 * kWGr, "rows of more than 4096 units are not supported");
    const RankWs w = carve_ws(tb, B, ws);
    float *S = w.S;
    hipStream_t st = (hipStream_t)stream;
    const bool head = mode == MKB_MODE_HEAD;
    // count the filtered ranks on S (and hand the finished scores out when asked)
    auto finish = [&](float f0, float f1, int64_t ld) {
        hipLaunchKernelGGL(rank_kernel, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, st, S, sample, (int)B, tb->n_entity,
                           tb->n_relation, head ? 1 : 0, true_keys, n_true, rank, f0, f1, ld);
        if (scores)
            hipLaunchKernelGGL(export_scores_kernel, dim3((unsigned)std::min<int64_t>((tb->n_entity + 255) / 256, 64), (unsigned)B), dim3(256), 0, st,
                               S, scores, tb->n_entity, ld, f0, f1);
    };
    return dispatch_model_side(tb->model, head, [&](auto m, auto h) { return run_rank<m(), h()>(tb, sample, B, w.Q, S, w.ids, st, finish); });
}

extern "C" int mkb_rank(const mkb_tables_t *tb, const int64_t *sample, int64_t B, int mode, const int64_t *true_keys,
                        int64_t n_true, int64_t *rank, void *ws, int64_t ws_bytes, void *stream) {
    return rank_impl(tb, sample, B, mode, true_keys, n_true, rank, nullptr, ws, ws_bytes, stream);
}

extern "C" int mkb_rank_scores(const mkb_tables_t *tb, const int64_t *sample, int64_t B, int mode, const int64_t *true_keys,
                               int64_t n_true, int64_t *rank, float *scores, void *ws, int64_t ws_bytes, void *stream) {
    MKB_REQUIRE(scores, "null pointer");
    return rank_impl(tb, sample, B, mode, true_keys, n_true, rank, scores, ws, ws_bytes, stream);
}

extern "C" int64_t mkb_topk_workspace_bytes(const mkb_tables_t *tb, int64_t B, int k) {
    if (k < 1 || k > MKB_TOPK_MAX_K) return 0;
    return mkb_rank_workspace_bytes(tb, B);
}

// mkb_topk and mkb_topk_masked (cand_bits == null: the kTopkPlain launch of mkb_topk itself)
static int topk_impl(const mkb_tables_t *tb, const int64_t *sample, int64_t B, int mode, const int64_t *true_keys, int64_t n_true,
                     const uint32_t *cand_bits, int k, int flags, int64_t *ids, float *scores, void *ws, int64_t ws_bytes, void *stream) {
    if (int rc = validate_tables(tb)) return rc;
    MKB_REQUIRE(sample && ids && scores && ws && (true_keys || n_true == 0) && n_true >= 0, "null pointer");
    MKB_REQUIRE(mode == MKB_MODE_HEAD || mode == MKB_MODE_TAIL, "mkb_topk needs head-batch or tail-batch");
    MKB_REQUIRE(k >= 1 && k <= MKB_TOPK_MAX_K, "k must lie in [1, %d]", MKB_TOPK_MAX_K);
    MKB_REQUIRE((flags & ~MKB_TOPK_KEEP_TARGET) == 0, "unknown flags");
    MKB_REQUIRE(B > 0 && B <= INT32_MAX, "bad B");
    MKB_REQUIRE(tb->n_entity <= INT32_MAX, "more than 2^31 - 1 entities");
    MKB_REQUIRE(ws_bytes >= mkb_topk_workspace_bytes(tb, B, k) && (((uintptr_t)ws) & 255) == 0, "workspace too small / unaligned");
    const int NU = tb->model == MKB_ROTATE ? tb->hidden_dim : (int)tb->entity_dim;
    MKB_REQUIRE(NU <= 4 * kWGr, "rows of more than 4096 units are not supported");
    const RankWs w = carve_ws(tb, B, ws);
    hipStream_t st = (hipStream_t)stream;
    const bool head = mode == MKB_MODE_HEAD;
    auto finish = [&](float f0, float f1, int64_t ld) {
        const TopkArgs A{w.S, sample, true_keys, ids, scores, B, tb->n_entity, tb->n_relation, n_true, ld, head ? 1 : 0, k,
                         (flags & MKB_TOPK_KEEP_TARGET) ? 1 : 0, f0, f1};
        const dim3 grid((unsigned)std::min<int64_t>(B, 1 << 20));  // (queries loop past the grid)
        if (cand_bits) {
            TopkMaskedArgs M;
            static_cast<TopkArgs &>(M) = A;
            M.cand = cand_bits;
            hipLaunchKernelGGL((topk_kernel<kTopkMasked, TopkMaskedArgs>), grid, dim3(kTopkThreads), 0, st, M);
        } else {
            hipLaunchKernelGGL(topk_kernel<kTopkPlain>, grid, dim3(kTopkThreads), 0, st, A);
        }
    };
    return dispatch_model_side(tb->model, head, [&](auto m, auto h) { return run_rank<m(), h()>(tb, sample, B, w.Q, w.S, w.ids, st, finish); });
}

extern "C" int mkb_topk(const mkb_tables_t *tb, const int64_t *sample, int64_t B, int mode, const int64_t *true_keys, int64_t n_true,
                        int k, int flags, int64_t *ids, float *scores, void *ws, int64_t ws_bytes, void *stream) {
    return topk_impl(tb, sample, B, mode, true_keys, n_true, nullptr, k, flags, ids, scores, ws, ws_bytes, stream);
}

extern "C" int mkb_topk_masked(const mkb_tables_t *tb, const int64_t *sample, int64_t B, int mode, const int64_t *true_keys,
                               int64_t n_true, const uint32_t *cand_bits, int k, int flags, int64_t *ids, float *scores, void *ws,
                               int64_t ws_bytes, void *stream) {
    return topk_impl(tb, sample, B, mode, true_keys, n_true, cand_bits, k, flags, ids, scores, ws, ws_bytes, stream);
}

extern "C" int mkb_topk_block(const float *S, int64_t B, int64_t N, int64_t ld, int k, int64_t *ids, float *scores, void *stream) {
    MKB_REQUIRE(S && ids && scores, "null pointer");
    MKB_REQUIRE(k >= 1 && k <= MKB_TOPK_MAX_K, "k must lie in [1, %d]", MKB_TOPK_MAX_K);
    MKB_REQUIRE(B >= 0 && B <= INT32_MAX, "bad B");
    MKB_REQUIRE(N >= 1 && N <= INT32_MAX, "N must lie in [1, 2^31 - 1]");
    MKB_REQUIRE(ld >= N, "ld must be >= N");
    if (B == 0) return MKB_OK;
    TopkArgs A{S, nullptr, nullptr, ids, scores, B, N, 0, 0, ld, 0, k, 0, 0.f, 1.f};
    hipLaunchKernelGGL(topk_kernel<kTopkBlock>, dim3((unsigned)std::min<int64_t>(B, 1 << 20)), dim3(kTopkThreads), 0, (hipStream_t)stream, A);
    MKB_LAUNCH_CHECK();
    return MKB_OK;
}

// Queries per pass of mkb_topk_nearest: the [rows, n_cand] distance block of one pass is about 2^24 floats (64 MB; 1,152 queries at
// FB15k-237's 14,541 candidates), a multiple of the tile's 64 rows and at least 64 of them.
static int64_t nearest_rows(int64_t B, int64_t n_cand) {
    const int64_t r = ((int64_t)1 << 24) / n_cand / kTileRows * kTileRows;
    return std::min(B, std::max<int64_t>(r, kTileRows));
}

extern "C" int64_t mkb_topk_nearest_workspace_bytes(int64_t B, int64_t n_cand, int k) {
    if (k < 1 || k > MKB_TOPK_MAX_K || B <= 0 || B > INT32_MAX || n_cand < 1 || n_cand > INT32_MAX) return 0;
    return (int64_t)(((size_t)nearest_rows(B, n_cand) * (size_t)n_cand * 4 + 255) & ~(size_t)255);
}

// mkb_topk_nearest (block == null) and mkb_topk_nearest_dists: per pass of `rows` queries the distance block S [b, n_cand] in the
// workspace (register tile or general route), its copy into block, and the kTopkNearest selection on it
static int nearest_impl(const float *Q, int64_t ldq, const float *X, int64_t ldx, const int64_t *cand, int64_t n_cand, int64_t B,
                        int64_t D, int k, int64_t *ids, float *dists, float *block, void *ws, int64_t ws_bytes, void *stream) {
    MKB_REQUIRE(Q && X && cand && ids && dists, "null pointer");
    MKB_REQUIRE(k >= 1 && k <= MKB_TOPK_MAX_K, "k must lie in [1, %d]", MKB_TOPK_MAX_K);
    MKB_REQUIRE(B >= 0 && B <= INT32_MAX, "bad B");
    MKB_REQUIRE(n_cand >= 1 && n_cand <= INT32_MAX, "n_cand must lie in [1, 2^31 - 1]");
    MKB_REQUIRE(D >= 1 && ldq >= D && ldx >= D, "need D >= 1, ldq >= D and ldx >= D");
    if (B == 0) return MKB_OK;
    MKB_REQUIRE(ws && ws_bytes >= mkb_topk_nearest_workspace_bytes(B, n_cand, k) && (((uintptr_t)ws) & 255) == 0,
                "workspace too small / unaligned");
    hipStream_t st = (hipStream_t)stream;
    float *S = (float *)ws;
    const int64_t rows = nearest_rows(B, n_cand);
    // the register tile reads rows of D floats, D apart, as float4 (S: the 256-byte aligned workspace)
    const bool tile = D % 4 == 0 && D >= 64 && D <= INT32_MAX && ldq == D && ldx == D && n_cand < (1 << 30) &&
                      (((uintptr_t)Q | (uintptr_t)X) & 15) == 0;
    for (int64_t lo = 0; lo < B; lo += rows) {
        const int64_t b = std::min(rows, B - lo);
        const float *q = Q + lo * ldq;
        if (tile) {  // the pooled forward's register tile, the candidate list as its pool (64 queries x 64 candidates per workgroup)
            PoolArgs P{};
            P.ent = X; P.Q = q; P.pool = cand; P.B = (int)b; P.P = (int)n_cand; P.De = D;
            TileArgs T{};
            T.part = S; T.Kd = (int)n_cand; T.ks = 1;
            T.row_tiles = (int)((b + kTileRows - 1) / kTileRows); T.pos_tiles = (int)((n_cand + kTilePos - 1) / kTilePos);
            hipLaunchKernelGGL((pool_fwd_tile_kernel<kTileL2, false, 2>), dim3((unsigned)T.row_tiles * (unsigned)T.pos_tiles), dim3(256), 0,
                               st, P, T);
        } else {
            hipLaunchKernelGGL(l2_block_kernel, dim3((unsigned)((n_cand + 255) / 256), (unsigned)std::min<int64_t>(b, 1024)), dim3(256), 0,
                               st, q, ldq, X, ldx, cand, n_cand, b, D, S);
        }
        if (block) MKB_CHECK_HIP(hipMemcpyAsync(block + lo * n_cand, S, (size_t)b * (size_t)n_cand * 4, hipMemcpyDeviceToDevice, st));
        TopkNearestArgs A;
        static_cast<TopkArgs &>(A) = TopkArgs{S, nullptr, nullptr, ids + lo * k, dists + lo * k, b, n_cand, 0, 0, n_cand, 0, k, 0, 0.f, 1.f};
        A.cand = cand;
        hipLaunchKernelGGL((topk_kernel<kTopkNearest, TopkNearestArgs>), dim3((unsigned)std::min<int64_t>(b, 1 << 20)), dim3(kTopkThreads),
                           0, st, A);
    }
    MKB_LAUNCH_CHECK();
    return MKB_OK;
}

extern "C" int mkb_topk_nearest(const float *Q, int64_t ldq, const float *X, int64_t ldx, const int64_t *cand, int64_t n_cand, int64_t B,
                                int64_t D, int k, int64_t *ids, float *dists, void *ws, int64_t ws_bytes, void *stream) {
    return nearest_impl(Q, ldq, X, ldx, cand, n_cand, B, D, k, ids, dists, nullptr, ws, ws_bytes, stream);
}

extern "C" int mkb_topk_nearest_dists(const float *Q, int64_t ldq, const float *X, int64_t ldx, const int64_t *cand, int64_t n_cand,
                                      int64_t B, int64_t D, int k, int64_t *ids, float *dists, float *block, void *ws, int64_t ws_bytes,
                                      void *stream) {
    MKB_REQUIRE(block, "null pointer");
    return nearest_impl(Q, ldq, X, ldx, cand, n_cand, B, D, k, ids, dists, block, ws, ws_bytes, stream);
}
