// The candidate-sorted pair list (pair_sort.h): the one place that instantiates hipCUB's radix sort.
#include <hipcub/hipcub.hpp>

#include "pair_sort.h"
#include "score_row.h"  // table_row

namespace mkb {

__global__ __launch_bounds__(256) void pair_keys_kernel(PairKeySegs S, int n, int *__restrict__ keys, int *__restrict__ vals) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    int64_t j = i;
    int s = 0;
    while (s + 1 < S.n_segs && j >= S.seg[s].n) j -= S.seg[s++].n;
    const PairKeySeg &g = S.seg[s];
    keys[i] = g.base + (int)table_row(g.ids[j * g.stride], g.n_table);
    vals[i] = i;
}

int pair_sort_plan(int64_t n_table, int64_t n_pairs, PairSortPlan &plan) {
    plan.bits = 1;
    while (plan.bits < 31 && ((int64_t)1 << plan.bits) < n_table) ++plan.bits;
    plan.sort_bytes = 0;
    MKB_CHECK_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, plan.sort_bytes, (const int *)nullptr, (int *)nullptr, (const int *)nullptr,
                                                     (int *)nullptr, (int)n_pairs, 0, plan.bits, (hipStream_t)0));
    plan.l_bytes = ((size_t)n_pairs * 4 + 255) & ~(size_t)255;
    plan.total = 4 * plan.l_bytes + ((plan.sort_bytes + 255) & ~(size_t)255);
    return MKB_OK;
}

int pair_sort_launch(const int64_t *cand, int64_t n_pairs, int64_t n_table, void *scratch, const PairSortPlan &plan, hipStream_t st,
                     const int **sorted_cand, const int **sorted_pair) {
    PairKeySegs one{};
    one.seg[0] = PairKeySeg{cand, 1, n_pairs, n_table, 0};
    one.n_segs = 1;
    return pair_sort_launch_segs(one, scratch, plan, st, sorted_cand, sorted_pair);
}

int pair_sort_launch_segs(const PairKeySegs &segs, void *scratch, const PairSortPlan &plan, hipStream_t st, const int **sorted_cand,
                          const int **sorted_pair) {
    int64_t n_pairs = 0;
    for (int s = 0; s < segs.n_segs; ++s) n_pairs += segs.seg[s].n;
    unsigned char *buf = (unsigned char *)scratch;
    int *k_in = (int *)buf, *v_in = (int *)(buf + plan.l_bytes), *k_out = (int *)(buf + 2 * plan.l_bytes),
        *v_out = (int *)(buf + 3 * plan.l_bytes);
    size_t sort_bytes = plan.sort_bytes;
    hipLaunchKernelGGL(pair_keys_kernel, dim3((unsigned)((n_pairs + 255) / 256)), dim3(256), 0, st, segs, (int)n_pairs, k_in, v_in);
    MKB_CHECK_HIP(hipcub::DeviceRadixSort::SortPairs(buf + 4 * plan.l_bytes, sort_bytes, k_in, k_out, v_in, v_out, (int)n_pairs, 0,
                                                     plan.bits, st));
    *sorted_cand = k_out;
    *sorted_pair = v_out;
    return MKB_OK;
}

}  // namespace mkb
