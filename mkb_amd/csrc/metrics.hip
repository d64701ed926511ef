// The two reductions behind the grouped evaluation report (evaluation.Evaluation.types_relations / detail_metrics /
// eval_per_relation; reference evaluation/evaluation.py:282-464): per-relation fan-out counts from the true triples and their
// sorted keys, and per-group rank metrics from the rank tensor Evaluation.ranks leaves on the device.  Integer atomics and a
// fixed-order double sum only: both results are bit-identical from run to run.
#include "common.h"

namespace mkb {

constexpr int kFanoutThreads = 256;
constexpr int kFanoutMaxBlocks = 1024;
constexpr int64_t kFanoutLdsRelations = 4096;  // 3 * 4096 uint32 counters = 48 KB of LDS; above that: global atomics directly

// Item i of the concatenation [triples | head keys | tail keys] adds one to counts[r][0 | 1 | 2]:
//   a triple to its relation's column 0 (every occurrence counts);
//   a key whose pair `key / N` differs from its predecessor's (or that is the first key) to column 1 (head keys: a new (t, r)
//   pair) or 2 (tail keys: a new (h, r) pair) of relation (key / N) % R.  The keys are ascending, so the keys of one pair are
//   contiguous and each pair is counted once.
// LDS = true: the workgroup counts in 3 * R uint32 of LDS (a workgroup sees fewer than 2^32 items) and adds its non-zero
// counters to the output once.  Ids outside [0, R) (and negative keys) are left out: nothing is indexed by them.
template <bool LDS>
__global__ __launch_bounds__(kFanoutThreads) void relation_fanout_kernel(const int64_t *__restrict__ triples, int64_t n,
                                                                         const int64_t *__restrict__ head_keys, int64_t n_head,
                                                                         const int64_t *__restrict__ tail_keys, int64_t n_tail,
                                                                         int64_t N, int64_t R, unsigned long long *__restrict__ counts) {
    extern __shared__ unsigned int s_cnt[];
    if (LDS) {
        for (int64_t j = threadIdx.x; j < 3 * R; j += kFanoutThreads) s_cnt[j] = 0u;
        __syncthreads();
    }
    const int64_t total = n + n_head + n_tail;
    for (int64_t i = (int64_t)blockIdx.x * kFanoutThreads + threadIdx.x; i < total; i += (int64_t)gridDim.x * kFanoutThreads) {
        int64_t r = -1;
        int col = 0;
        if (i < n) {
            r = triples[3 * i + 1];
        } else {
            const bool head = i < n + n_head;
            const int64_t *__restrict__ keys = head ? head_keys : tail_keys;
            const int64_t j = head ? i - n : i - n - n_head;
            const int64_t key = keys[j];
            const int64_t pair = key / N;
            if (key >= 0 && (j == 0 || keys[j - 1] / N != pair)) r = pair % R;
            col = head ? 1 : 2;
        }
        if (r >= 0 && r < R) {
            if (LDS) atomicAdd(&s_cnt[3 * r + col], 1u);
            else atomicAdd(&counts[3 * r + col], 1ull);
        }
    }
    if (LDS) {
        __syncthreads();
        for (int64_t j = threadIdx.x; j < 3 * R; j += kFanoutThreads)
            if (s_cnt[j]) atomicAdd(&counts[j], (unsigned long long)s_cnt[j]);
    }
}

constexpr int kMetricThreads = 256;

// Workgroup g reduces the items of group g: item i belongs to group_of_relation[sample[i][1]] (negative, or a relation id
// outside the table: to none).  Lane l takes items l, l + 256, ... in that order; the 256 partial results are then added
// pairwise in LDS (stride 128, 64, ..., 1).  The order is a function of n alone, so the double sum is reproducible.
__global__ __launch_bounds__(kMetricThreads) void rank_metrics_kernel(const int64_t *__restrict__ ranks, const int64_t *__restrict__ sample,
                                                                      int64_t n, const int32_t *__restrict__ group_of_relation, int64_t R,
                                                                      int64_t *__restrict__ counts, double *__restrict__ rr_sum) {
    __shared__ int64_t s_int[5][kMetricThreads];
    __shared__ double s_rr[kMetricThreads];
    const int g = (int)blockIdx.x, lane = (int)threadIdx.x;
    int64_t cnt = 0, sum = 0, h1 = 0, h3 = 0, h10 = 0;
    double rr = 0.0;
    for (int64_t i = lane; i < n; i += kMetricThreads) {
        const int64_t r = sample[3 * i + 1];
        if (r < 0 || r >= R || group_of_relation[r] != g) continue;
        const int64_t rank = ranks[i];
        cnt += 1;
        sum += rank;
        h1 += rank <= 1;
        h3 += rank <= 3;
        h10 += rank <= 10;
        rr += 1.0 / (double)rank;
    }
    s_int[0][lane] = cnt, s_int[1][lane] = sum, s_int[2][lane] = h1, s_int[3][lane] = h3, s_int[4][lane] = h10;
    s_rr[lane] = rr;
    __syncthreads();
    for (int off = kMetricThreads / 2; off > 0; off >>= 1) {
        if (lane < off) {
#pragma unroll
            for (int c = 0; c < 5; ++c) s_int[c][lane] += s_int[c][lane + off];
            s_rr[lane] += s_rr[lane + off];
        }
        __syncthreads();
    }
    if (lane < 5) counts[5 * (int64_t)g + lane] = s_int[lane][0];
    if (lane == 0) rr_sum[g] = s_rr[0];
}

}  // namespace mkb

extern "C" int mkb_relation_fanout(const int64_t *triples, int64_t n, const int64_t *head_keys, int64_t n_head,
                                   const int64_t *tail_keys, int64_t n_tail, int64_t n_entity, int64_t n_relation, int64_t *counts,
                                   void *stream) {
    MKB_REQUIRE(n_entity > 0 && n_relation > 0 && n_relation <= INT32_MAX, "bad table size (%lld entities, %lld relations)",
                (long long)n_entity, (long long)n_relation);
    MKB_REQUIRE(n >= 0 && n_head >= 0 && n_tail >= 0 && n <= INT64_MAX / 4 && n_head <= INT64_MAX / 4 && n_tail <= INT64_MAX / 4,
                "bad item count (%lld triples, %lld + %lld keys)", (long long)n, (long long)n_head, (long long)n_tail);
    MKB_REQUIRE(counts && (triples || n == 0) && (head_keys || n_head == 0) && (tail_keys || n_tail == 0), "null pointer");
    hipStream_t st = (hipStream_t)stream;
    MKB_CHECK_HIP(hipMemsetAsync(counts, 0, (size_t)n_relation * 3 * sizeof(int64_t), st));
    const int64_t total = n + n_head + n_tail;
    if (total == 0) return MKB_OK;
    const int64_t want = (total + mkb::kFanoutThreads - 1) / mkb::kFanoutThreads;
    const unsigned blocks = (unsigned)(want > mkb::kFanoutMaxBlocks ? mkb::kFanoutMaxBlocks : want);
    unsigned long long *out = reinterpret_cast<unsigned long long *>(counts);
    if (n_relation <= mkb::kFanoutLdsRelations)
        hipLaunchKernelGGL(mkb::relation_fanout_kernel<true>, dim3(blocks), dim3(mkb::kFanoutThreads),
                           (size_t)n_relation * 3 * sizeof(unsigned int), st, triples, n, head_keys, n_head, tail_keys, n_tail, n_entity,
                           n_relation, out);
    else
        hipLaunchKernelGGL(mkb::relation_fanout_kernel<false>, dim3(blocks), dim3(mkb::kFanoutThreads), 0, st, triples, n, head_keys,
                           n_head, tail_keys, n_tail, n_entity, n_relation, out);
    MKB_LAUNCH_CHECK();
    return MKB_OK;
}

extern "C" int mkb_rank_metrics(const int64_t *ranks, const int64_t *sample, int64_t n, const int32_t *group_of_relation,
                                int64_t n_relation, int n_groups, int64_t *counts, double *rr_sum, void *stream) {
    MKB_REQUIRE(n_relation > 0 && n_groups > 0, "bad table size (%lld relations, %d groups)", (long long)n_relation, n_groups);
    MKB_REQUIRE(n >= 0 && n <= INT64_MAX / 4, "bad item count %lld", (long long)n);
    MKB_REQUIRE(group_of_relation && counts && rr_sum && ((ranks && sample) || n == 0), "null pointer");
    hipLaunchKernelGGL(mkb::rank_metrics_kernel, dim3((unsigned)n_groups), dim3(mkb::kMetricThreads), 0, (hipStream_t)stream, ranks,
                       sample, n, group_of_relation, n_relation, counts, rr_sum);
    MKB_LAUNCH_CHECK();
    return MKB_OK;
}
