// The relation side of link prediction, (h, ?, t): mkb_rel_scores / mkb_rel_rank / mkb_rel_topk.
//
// Replaces evaluation.Evaluation.compute_score on the relation-batch stream (evaluation/evaluation.py:217-279 with the candidate
// list and bias of datasets.base.TestDatasetRelation, datasets/base.py:254-305) and the [b, R, 3] forward the glue ran for it: one
// general-forward workgroup per (h, r', t), each gathering the same two entity rows.
//
// Scores  : one workgroup per query.  The h and t rows are staged in LDS once; the relations go by in turns of 4: the workgroup
//           builds the four queries of (h, r') with the arithmetic of query_unit and stages each in an LDS row exactly as the
//           general forward stages its one query, then each of the 4 waves sums the pair terms of one of them against t with
//           the general forward's own loop (score_row.h) and finishes with wave_sum and finish_score: every score has the bits
//           mkb_score_fwd gives the same triple in default mode.  The relation rows stream from L2 (the table is small), the
//           two entity rows are the query's only other traffic.
// Filter  : one lane per (query, relation) looks (h * R + r') * N + t up in the sorted tail-batch keys -- for a fixed (h, t) the
//           keys of different relations are not contiguous, so it is a search per relation, not a range walk -- and a ballot
//           packs the hits into a bitmask [B, ceil(R / 32)].
// Rank    : one wave per query counts, in ranks_before order, the relations ahead of the target; a filtered relation stands at
//           the target's score - 1 (base.py:289-295), so it is behind the target unless the target's score is NaN or infinite.
// Top k   : one workgroup per query; each lane places the unfiltered relations it owns by counting those ahead of them (the
//           order is total, so the counts are the positions).  Quadratic in n_relation, which is a few hundred to a few
//           thousand; no atomics, nothing to sort.
// Nothing is allocated in a call and nothing is accumulated with atomics: two runs give the same bits.
//
// The score kernel is the slot forward: with a list per row it scores candidate relations or -- the heads varying, r and t the
// staged rows, the turn's four head rows from the entity table (default-mode arithmetic, query_of<MODEL, false>(h', r): not the
// head-batch kernels, whose order of operations gives other bits) -- candidate heads.  launch_slot_scores (score_slot.h) is how
// score_cand.hip reaches it; nothing here depends on the candidate-list entry points or on the general kernels.
#include "common.h"
#include "query_side.h"
#include "rank_order.h"
#include "score_row.h"
#include "score_slot.h"

#include <algorithm>

namespace mkb {

constexpr size_t kRelLdsMax = 64 * 1024;

// LDS of the score kernel: the h row, the t row and one query row per wave
static size_t rel_lds_bytes(const mkb_tables_t *tb) { return (size_t)(2 + kSlotWaves) * (size_t)tb->entity_dim * sizeof(float); }

int slot_rows_check(const mkb_tables_t *tb) {
    if (rel_lds_bytes(tb) > kRelLdsMax)
        return set_error(MKB_ERR_UNSUPPORTED, "entity rows of more than %d floats are not supported by the slot kernels",
                         (int)(kRelLdsMax / sizeof(float) / (2 + kSlotWaves)));
    return MKB_OK;
}

// query_of<MKB_COMPLEX, false>(e, r) with the contraction spelled out that the general forward's compilation of it has: the
// products with r.re fused, the other two rounded.  Left to the compiler, a loop in which r is the invariant operand (the heads
// vary) fuses the other product of q.im, and one score in a few differs from mkb_score_fwd's by an ulp.
__device__ __forceinline__ Cplx complex_query_of(Cplx e, Cplx r) {
    return Cplx{fmaf(e.re, r.re, -__fmul_rn(e.im, r.im)), fmaf(e.im, r.re, __fmul_rn(e.re, r.im))};
}

// The scores of row i's candidates in one slot of the triple.  VARY_HEAD = false: the candidates are relations, (h, r', t) -- the
// relation side's kernel; true: they are heads, (h', r, t), and r takes h's place as the staged operand of the query.
//   cand: row i's list is cand + i * cand_stride (stride 0: one list for the whole batch, mkb_rel_scores); null = the ids 0 ..
//   n_cand - 1.  n_table = the rows of the table the candidates index.
template <int MODEL, bool VARY_HEAD>
__global__ __launch_bounds__(kSlotBlock) void slot_score_kernel(TablesDev T, const int64_t *__restrict__ sample,
                                                               const int64_t *__restrict__ cand, int64_t cand_stride, int n_cand,
                                                               int64_t n_table, float *__restrict__ scores, int64_t ld) {
    extern __shared__ __attribute__((aligned(16))) float rel_lds[];
    float *s_a = rel_lds, *s_t = rel_lds + T.De;  // the query's fixed operand (h; r when the heads vary) and the tail
    const int64_t i = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float *q_lds = rel_lds + (2 + wave) * T.De;
    const int U = ModelTraits<MODEL>::cplx_query ? T.d : (int)T.De;  // units per row
    {
        // (the varying column is not read)
        const float *ea = VARY_HEAD ? T.rel + sample[3 * i + 1] * T.Dr : T.ent + sample[3 * i] * T.De;
        const float *et = T.ent + sample[3 * i + 2] * T.De;
        const int na = VARY_HEAD ? (int)T.Dr : (int)T.De;
        for (int k = threadIdx.x; k < (int)T.De; k += kSlotBlock) {
            if (!VARY_HEAD || k < na) s_a[k] = ea[k];
            s_t[k] = et[k];
        }
    }
    __syncthreads();
    const int64_t *list = cand ? cand + i * cand_stride : nullptr;
    const float modulus = (MODEL == MKB_PROTATE) ? T.modulus[0] : 0.f;
    const bool vec4 = T.vec4 != 0;
    for (int j0 = 0; j0 < n_cand; j0 += kSlotWaves) {  // a turn: kSlotWaves candidates, one per wave
        const int j = j0 + wave;
        // The turn's queries are built by the whole workgroup: a lane owns units, loads its unit of the fixed operand once and the
        // turn's candidate units together (independent loads in flight: one wave building its own candidate's query alone waited for
        // one row load per 64 units), then builds each with the arithmetic of query_unit.  (Past the last candidate: the last one
        // again, not used.)
        const float *ec[kSlotWaves];
#pragma unroll
        for (int w = 0; w < kSlotWaves; ++w) {
            const int jw = min(j0 + w, n_cand - 1);
            const int64_t id = table_row(list ? list[jw] : (int64_t)jw, n_table);
            ec[w] = VARY_HEAD ? T.ent + id * T.De : T.rel + id * T.Dr;
        }
        for (int u = threadIdx.x; u < U; u += kSlotBlock) {
            if constexpr (ModelTraits<MODEL>::cplx_query) {
                const Cplx a = VARY_HEAD ? rel_unit<MODEL>(s_a, T.d, u) : ent_unit(s_a, T.d, u);
                Cplx c[kSlotWaves];
#pragma unroll
                for (int w = 0; w < kSlotWaves; ++w) c[w] = VARY_HEAD ? ent_unit(ec[w], T.d, u) : rel_unit<MODEL>(ec[w], T.d, u);
#pragma unroll
                for (int w = 0; w < kSlotWaves; ++w) {
                    Cplx q;
                    if constexpr (VARY_HEAD && MODEL == MKB_COMPLEX) q = complex_query_of(c[w], a);
                    else q = VARY_HEAD ? query_of<MODEL, false>(c[w], a, T.kd) : query_of<MODEL, false>(a, c[w], T.kd);
                    rel_lds[(2 + w) * T.De + u] = q.re;
                    rel_lds[(2 + w) * T.De + T.d + u] = q.im;
                }
            } else {
                const float a = s_a[u];
                float c[kSlotWaves];
#pragma unroll
                for (int w = 0; w < kSlotWaves; ++w) c[w] = ec[w][u];
#pragma unroll
                for (int w = 0; w < kSlotWaves; ++w)
                    rel_lds[(2 + w) * T.De + u] = VARY_HEAD ? query_of<MODEL, false>(c[w], a, T.kd) : query_of<MODEL, false>(a, c[w], T.kd);
            }
        }
        __syncthreads();
        if (j < n_cand) {
            float acc = pair_row_sum<MODEL, false>(T, q_lds, s_t, lane, vec4);
            acc = wave_sum(acc);
            if (lane == 0) scores[i * ld + j] = finish_score<MODEL>(acc, T.gamma, modulus);
        }
        __syncthreads();
    }
}

// mask[i * W + w] bit b = (h_i, 32 w + b, t_i) is a key.  One wave per (query, 64 relations); every word of the mask is written.
__global__ __launch_bounds__(256) void rel_filter_kernel(const int64_t *__restrict__ sample, int64_t B, int64_t R, int64_t N,
                                                         const int64_t *__restrict__ keys, int64_t nk, uint32_t *__restrict__ mask,
                                                         int64_t W) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t chunks = (R + 63) / 64;
    for (int64_t w = (int64_t)blockIdx.x * 4 + wave; w < B * chunks; w += (int64_t)gridDim.x * 4) {
        const int64_t i = w / chunks, c = w % chunks, r = c * 64 + lane;
        bool hit = false;
        if (r < R) {
            const int64_t want = (sample[3 * i] * R + r) * N + sample[3 * i + 2];
            int64_t lo = 0, hi = nk;
            while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (keys[mid] < want) lo = mid + 1; else hi = mid; }
            hit = lo < nk && keys[lo] == want;
        }
        const uint64_t m = __ballot(hit);
        if (lane == 0) {
            mask[i * W + 2 * c] = (uint32_t)m;
            if (2 * c + 1 < W) mask[i * W + 2 * c + 1] = (uint32_t)(m >> 32);
        }
    }
}

// one wave per query
__global__ __launch_bounds__(256) void rel_rank_kernel(const float *__restrict__ S, int64_t ld, const uint32_t *__restrict__ mask,
                                                       int64_t W, const int64_t *__restrict__ sample, int64_t B, int64_t R,
                                                       int64_t *__restrict__ rank) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int64_t i = (int64_t)blockIdx.x * 4 + wave; i < B; i += (int64_t)gridDim.x * 4) {
        const int64_t r = sample[3 * i + 1];
        const float *row = S + i * ld;
        const uint32_t *bits = mask + i * W;
        const float st = row[r], biased = st + (-1.0f);
        int64_t cnt = 0;
        for (int64_t e = lane; e < R; e += 64) {
            const bool filtered = ((bits[e >> 5] >> (e & 31)) & 1u) != 0u;
            const float v = filtered ? biased : row[e];
            cnt += (e != r && ranks_before(v, e, st, r)) ? 1 : 0;
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off, 64);
        if (lane == 0) rank[i] = cnt + 1;
    }
}

// one workgroup per query
__global__ __launch_bounds__(256) void rel_topk_kernel(const float *__restrict__ S, int64_t ld, const uint32_t *__restrict__ mask,
                                                       int64_t W, const int64_t *__restrict__ sample, int64_t B, int64_t R, int k,
                                                       int keep_target, int64_t *__restrict__ ids, float *__restrict__ scores) {
    __shared__ int s_n[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int64_t i = blockIdx.x; i < B; i += gridDim.x) {
        const int64_t keep = keep_target ? sample[3 * i + 1] : -1;
        const float *row = S + i * ld;
        const uint32_t *bits = mask + i * W;
        auto cand = [&](int64_t e) { return e == keep || ((bits[e >> 5] >> (e & 31)) & 1u) == 0u; };
        int mine = 0;
        for (int64_t e = tid; e < R; e += 256) {
            if (!cand(e)) continue;
            const float v = row[e];
            int64_t pos = 0;
            for (int64_t f = 0; f < R; ++f) pos += (f != e && cand(f) && ranks_before(row[f], f, v, e)) ? 1 : 0;
            ++mine;
            if (pos < k) {
                ids[i * k + pos] = e;
                scores[i * k + pos] = v;
            }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) mine += __shfl_xor(mine, off, 64);
        if (lane == 0) s_n[wave] = mine;
        __syncthreads();
        const int n = s_n[0] + s_n[1] + s_n[2] + s_n[3];  // the candidates left: the slots past them are padding
        for (int j = n + tid; j < k; j += 256) {
            ids[i * k + j] = -1;
            scores[i * k + j] = -INFINITY;
        }
        __syncthreads();
    }
}

int launch_slot_scores(const mkb_tables_t *tb, const int64_t *sample, int64_t B, const int64_t *cand, int64_t cand_stride, int64_t n_cand,
                       bool vary_head, float *scores, int64_t ld, hipStream_t st) {
    const TablesDev T = to_dev(tb);
    const size_t lds = rel_lds_bytes(tb);
    const dim3 grid((unsigned)B), block(kSlotBlock);
    const int64_t n_table = vary_head ? tb->n_entity : tb->n_relation;
    return dispatch_model_side(tb->model, vary_head, [&](auto m, auto vh) {
        hipLaunchKernelGGL((slot_score_kernel<m(), vh()>), grid, block, lds, st, T, sample, cand, cand_stride, (int)n_cand, n_table, scores, ld);
        return (int)MKB_OK;
    });
}

// rel_ids: one list of n_rel relations for every query (null: all of them in order)
static int launch_scores(const mkb_tables_t *tb, const int64_t *sample, int64_t B, const int64_t *rel_ids, int64_t n_rel, float *scores,
                         int64_t ld, hipStream_t st) {
    return launch_slot_scores(tb, sample, B, rel_ids, 0, n_rel, false, scores, ld, st);
}

static int64_t mask_words(const mkb_tables_t *tb) { return (tb->n_relation + 31) / 32; }
static size_t block_bytes(const mkb_tables_t *tb, int64_t B) { return ((size_t)B * (size_t)tb->n_relation * 4 + 255) & ~(size_t)255; }

// what mkb_rel_rank and mkb_rel_topk share: the checks of their common arguments, in the order of the ABI
static int check_rel_call(const mkb_tables_t *tb, const int64_t *sample, int64_t B, const int64_t *true_keys, int64_t n_true, void *ws,
                          int64_t ws_bytes, int64_t need) {
    MKB_REQUIRE(sample != nullptr, "sample is null");
    MKB_REQUIRE(B >= 0 && B <= INT32_MAX, "B must lie in [0, 2^31 - 1]");
    MKB_REQUIRE(n_true >= 0 && (true_keys != nullptr || n_true == 0), "n_true > 0 needs true_keys");
    MKB_REQUIRE(tb->n_relation <= INT32_MAX, "more than 2^31 - 1 relations");
    MKB_REQUIRE(B == 0 || (ws != nullptr && (((uintptr_t)ws) & 255) == 0 && ws_bytes >= need), "workspace null, too small or unaligned");
    return slot_rows_check(tb);
}

// block (null: the workspace's) = the [B, n_relation] scores, then the filter mask behind the workspace's block
static void launch_block_and_mask(const mkb_tables_t *tb, const int64_t *sample, int64_t B, const int64_t *true_keys, int64_t n_true,
                                  float *S, uint32_t *mask, hipStream_t st) {
    launch_scores(tb, sample, B, nullptr, tb->n_relation, S, tb->n_relation, st);
    const int64_t waves = B * ((tb->n_relation + 63) / 64);
    hipLaunchKernelGGL(rel_filter_kernel, dim3((unsigned)std::min<int64_t>((waves + 3) / 4, 1 << 20)), dim3(256), 0, st, sample, B,
                       tb->n_relation, tb->n_entity, true_keys, n_true, mask, mask_words(tb));
}

}  // namespace mkb

using namespace mkb;

extern "C" int mkb_rel_scores(const mkb_tables_t *tb, const int64_t *sample, int64_t B, const int64_t *rel_ids, int64_t n_rel,
                              float *scores, int64_t ld, void *stream) {
    if (int rc = validate_tables(tb)) return rc;
    MKB_REQUIRE(sample != nullptr && scores != nullptr, "null pointer");
    MKB_REQUIRE(B >= 0 && B <= INT32_MAX, "B must lie in [0, 2^31 - 1]");
    MKB_REQUIRE(n_rel >= 1 && n_rel <= INT32_MAX, "n_rel must lie in [1, 2^31 - 1]");
    MKB_REQUIRE(rel_ids != nullptr || n_rel == tb->n_relation, "null rel_ids means every relation: n_rel must equal n_relation");
    MKB_REQUIRE(ld >= n_rel, "ld must be >= n_rel");
    if (int rc = slot_rows_check(tb)) return rc;
    if (B == 0) return MKB_OK;
    if (int rc = launch_scores(tb, sample, B, rel_ids, n_rel, scores, ld, (hipStream_t)stream)) return rc;
    MKB_LAUNCH_CHECK();
    return MKB_OK;
}

extern "C" int64_t mkb_rel_rank_workspace_bytes(const mkb_tables_t *tb, int64_t B) {
    if (!tb || B <= 0 || B > INT32_MAX || tb->n_relation <= 0 || tb->n_relation > INT32_MAX) return 0;
    return (int64_t)block_bytes(tb, B) + (int64_t)(((size_t)B * (size_t)mask_words(tb) * 4 + 255) & ~(size_t)255);
}

extern "C" int mkb_rel_rank(const mkb_tables_t *tb, const int64_t *sample, int64_t B, const int64_t *true_keys, int64_t n_true,
                            int64_t *rank, float *scores, void *ws, int64_t ws_bytes, void *stream) {
    if (int rc = validate_tables(tb)) return rc;
    MKB_REQUIRE(rank != nullptr, "rank is null");
    if (int rc = check_rel_call(tb, sample, B, true_keys, n_true, ws, ws_bytes, mkb_rel_rank_workspace_bytes(tb, B))) return rc;
    if (B == 0) return MKB_OK;
    hipStream_t st = (hipStream_t)stream;
    float *S = scores ? scores : (float *)ws;  // a caller's block is the block the ranks are counted on
    uint32_t *mask = (uint32_t *)((unsigned char *)ws + block_bytes(tb, B));
    launch_block_and_mask(tb, sample, B, true_keys, n_true, S, mask, st);
    hipLaunchKernelGGL(rel_rank_kernel, dim3((unsigned)std::min<int64_t>((B + 3) / 4, 1 << 20)), dim3(256), 0, st, S, tb->n_relation, mask,
                       mask_words(tb), sample, B, tb->n_relation, rank);
    MKB_LAUNCH_CHECK();
    return MKB_OK;
}

extern "C" int64_t mkb_rel_topk_workspace_bytes(const mkb_tables_t *tb, int64_t B, int k) {
    if (k < 1 || k > MKB_TOPK_MAX_K) return 0;
    return mkb_rel_rank_workspace_bytes(tb, B);
}

extern "C" int mkb_rel_topk(const mkb_tables_t *tb, const int64_t *sample, int64_t B, const int64_t *true_keys, int64_t n_true, int k,
                            int flags, int64_t *ids, float *scores, void *ws, int64_t ws_bytes, void *stream) {
    if (int rc = validate_tables(tb)) return rc;
    MKB_REQUIRE(ids != nullptr && scores != nullptr, "null pointer");
    MKB_REQUIRE(k >= 1 && k <= MKB_TOPK_MAX_K, "k must lie in [1, %d]", MKB_TOPK_MAX_K);
    MKB_REQUIRE((flags & ~MKB_TOPK_KEEP_TARGET) == 0, "unknown flags");
    if (int rc = check_rel_call(tb, sample, B, true_keys, n_true, ws, ws_bytes, mkb_rel_topk_workspace_bytes(tb, B, k))) return rc;
    if (B == 0) return MKB_OK;
    hipStream_t st = (hipStream_t)stream;
    float *S = (float *)ws;
    uint32_t *mask = (uint32_t *)((unsigned char *)ws + block_bytes(tb, B));
    launch_block_and_mask(tb, sample, B, true_keys, n_true, S, mask, st);
    hipLaunchKernelGGL(rel_topk_kernel, dim3((unsigned)std::min<int64_t>(B, 1 << 20)), dim3(256), 0, st, S, tb->n_relation, mask,
                       mask_words(tb), sample, B, tb->n_relation, k, (flags & MKB_TOPK_KEEP_TARGET) ? 1 : 0, ids, scores);
    MKB_LAUNCH_CHECK();
    return MKB_OK;
}
