// What the all-entity training steps share, written once: score_all.hip (ComplEx / DistMult, whose block is one matrix product) and
// score_all_dist.hip (TransE / RotatE / pRotatE, whose block is a sum of distances) both run
//   the loss kernels on a plain [B, ld] block (defined in score_all.hip; they know nothing of the model), and
//   the query chain: dQ [B, De] -> the query's entity row and relation row, one writer per distinct row, for any of the five models
//   (query_side.h, model_math.h).
#pragma once
#include "common.h"
#include "pair_sort.h"
#include "query_side.h"

namespace mkb {

inline size_t up256(size_t n) { return (n + 255) & ~(size_t)255; }

// ---- the loss kernels on the block (score_all.hip): S [B, ld] is overwritten with dS, pad columns N .. ld - 1 with exactly 0
void all_softmax_launch(float *S, int64_t B, int64_t N, int64_t ld, const int64_t *target, int64_t tstride, const float *weight,
                        const float *weight_sum, float T, float *loss, float *pos, float *scratch, hipStream_t st);
void all_bce_launch(float *S, int64_t B, int64_t N, int64_t ld, const int64_t *sample, bool head, int64_t R, const int64_t *keys,
                    int64_t n_keys, const float *weight, const float *weight_sum, float eps, bool sum_over_entities, float *loss,
                    float *pos, float *scratch, hipStream_t st);
void all_softmax_filtered_launch(float *S, int64_t B, int64_t N, int64_t ld, const int64_t *target, int64_t tstride,
                                 const int64_t *sample, bool head, int64_t R, const int64_t *keys, int64_t n_keys, const float *weight,
                                 const float *weight_sum, float T, float eps, float *loss, float *pos, float *scratch, hipStream_t st);
// ... and the argument checks of the entry points around them
int softmax_check(const void *S, int64_t B, int64_t N, int64_t ld, const void *target, int64_t tstride, float T, const void *loss,
                  const void *pos, const void *scratch);
int bce_check(int64_t N, int64_t R, int mode, const void *keys, int64_t n_keys, float eps, const char *what = "KvsAll");

// ---- query chain: dQ -> the query's entity row (h; t for head-batch) and relation row, one writer per distinct row
struct ChainArgs {
    const float *ent, *rel;  // (the table fields query_row reads)
    int64_t De, Dr;
    int d;
    float kd;
    const int64_t *sample;
    const float *dQ;
    float *g_ent, *g_rel;
    const int *keys, *vals;  // the sorted occurrences: row keys (relations: n_entity + r) and occurrence indices (relations: B + i)
    int n, B, n_entity;
    float *stash;  // [B, De]: what the gradient rows of the batch's query entities held before the step, by sorted position
};

// The gradient row of a query's entity takes two terms, its row of the product dE and the chain's.  Adding them one after the other
// onto what the row already holds would round twice; so the row's content is set aside and the row cleared here, the product adds
// onto zero (exact), and the chain kernel writes stash + (product + chain): the finished result is added once, as for every
// other row.  One workgroup per sorted position of the entity keys (they sort in front of the relation keys: positions 0 .. B - 1).
static __global__ __launch_bounds__(256) void all_stash_kernel(ChainArgs A) {
    const int pos = blockIdx.x;
    const int key = A.keys[pos];
    if (pos > 0 && A.keys[pos - 1] == key) return;
    float *g = A.g_ent + (int64_t)key * A.De, *x = A.stash + (int64_t)pos * A.De;
    for (int64_t u = threadIdx.x; u < A.De; u += 256) {
        x[u] = g[u];
        g[u] = 0.f;
    }
}

template <int MODEL, bool HEAD>
__global__ __launch_bounds__(256) void all_chain_kernel(ChainArgs A) {
    constexpr bool CQ = ModelTraits<MODEL>::cplx_query;
    const int pos = blockIdx.x;
    const int key = A.keys[pos];
    if (pos > 0 && A.keys[pos - 1] == key) return;  // (uniform) only the position that opens a run of equal keys owns the row
    const bool is_rel = key >= A.n_entity;
    float *g = is_rel ? A.g_rel + (int64_t)(key - A.n_entity) * A.Dr : A.g_ent + (int64_t)key * A.De;
    const bool has_im = CQ && (!is_rel || MODEL == MKB_COMPLEX);
    const int U = CQ ? A.d : (int)A.De;
    for (int u = threadIdx.x; u < U; u += 256) {
        float a_re = 0.f, a_im = 0.f;
        for (int j = pos; j < A.n && A.keys[j] == key; ++j) {  // the run in batch order (the sort is stable)
            const int64_t i = A.vals[j] % A.B;
            const QueryRow R = query_row<MODEL>(A, A.sample, i);
            const float *dq = A.dQ + i * A.De;
            const float dq0 = dq[u], dq1 = CQ ? dq[A.d + u] : 0.f;
            Cplx de, dr;
            query_unit_bwd<MODEL, HEAD>(R, u, dq0, dq1, de, dr);
            a_re += is_rel ? dr.re : de.re;
            a_im += is_rel ? dr.im : de.im;
        }
        if (is_rel) {
            g[u] += a_re;
            if (has_im) g[A.d + u] += a_im;
        } else {  // (see all_stash_kernel)
            const float *x = A.stash + (int64_t)pos * A.De;
            g[u] = x[u] + (g[u] + a_re);
            if (has_im) g[A.d + u] = x[A.d + u] + (g[A.d + u] + a_im);
        }
    }
}

// Opens the chain in front of the product that writes dE: sorts the 2 B occurrences (the query's entity, then its relation) and sets
// the query entities' gradient rows aside (all_stash_kernel).  A: what all_chain_kernel is then launched with, over 2 B positions,
// once dQ and dE are there.
template <bool HEAD>
static int all_chain_open(const mkb_tables_t *tb, const mkb_grads_t *gr, const int64_t *sample, int64_t B, const float *dQ, float *stash,
                          void *sort, const PairSortPlan &plan, hipStream_t st, ChainArgs &A) {
    const int64_t N = tb->n_entity;
    PairKeySegs segs{};
    segs.seg[0] = PairKeySeg{sample + (HEAD ? 2 : 0), 3, B, N, 0};    // the query's entity
    segs.seg[1] = PairKeySeg{sample + 1, 3, B, tb->n_relation, (int)N};  // its relation
    segs.n_segs = 2;
    A = ChainArgs{};
    if (int rc = pair_sort_launch_segs(segs, sort, plan, st, &A.keys, &A.vals)) return rc;
    A.ent = tb->ent; A.rel = tb->rel; A.De = tb->entity_dim; A.Dr = tb->relation_dim; A.d = tb->hidden_dim; A.kd = tb->phase_div;
    A.sample = sample; A.dQ = dQ; A.g_ent = gr->g_ent; A.g_rel = gr->g_rel;
    A.n = (int)(2 * B); A.B = (int)B; A.n_entity = (int)N; A.stash = stash;
    hipLaunchKernelGGL(all_stash_kernel, dim3((unsigned)B), dim3(256), 0, st, A);
    return MKB_OK;
}

}  // namespace mkb
