// The candidate-sorted pair list of the candidate-list backward passes (score_general.hip's dx pass, score_cand.hip's candidate
// pass), made in pair_sort.hip: key = the candidate as a row of its table, value = the pair's index in [B, M]; one radix sort of
// n_pairs int32 keys.  The scratch is the caller's: the pair list twice (radix sort ping-pong), then the sort's own storage.
#pragma once
#include "common.h"

namespace mkb {

struct PairSortPlan {
    size_t l_bytes, sort_bytes, total;  // one list of the four, the sort's storage, all of the scratch (a multiple of 256)
    int bits;                           // the key bits the sort looks at: enough for n_table rows
};

// n_table and n_pairs below 2^31.  MKB_ERR_HIP if the sort's size query fails.
int pair_sort_plan(int64_t n_table, int64_t n_pairs, PairSortPlan &plan);

// cand [n_pairs] -> the pairs in candidate order, in `scratch` (256-byte aligned, plan.total bytes); an id outside the table
// sorts as the nearest row (table_row, score_row.h)
int pair_sort_launch(const int64_t *cand, int64_t n_pairs, int64_t n_table, void *scratch, const PairSortPlan &plan, hipStream_t st,
                     const int **sorted_cand, const int **sorted_pair);

// The same sort over a key list made of up to kPairKeySegs segments laid end to end (reg_rows.hip: the heads, the tails and the
// relations of a batch in one sort): pair first + j of a segment has the key base + table_row(ids[j * stride], n_table).  The
// plan is pair_sort_plan(the largest key + 1, the segments' total n); the sort is stable, so equal keys keep their pair order.
constexpr int kPairKeySegs = 3;
struct PairKeySeg {
    const int64_t *ids;
    int64_t stride, n, n_table;
    int base;
};
struct PairKeySegs {
    PairKeySeg seg[kPairKeySegs];
    int n_segs;
};
int pair_sort_launch_segs(const PairKeySegs &segs, void *scratch, const PairSortPlan &plan, hipStream_t st, const int **sorted_key,
                          const int **sorted_pair);

}  // namespace mkb
