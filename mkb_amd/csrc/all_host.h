// The host side of the all-entity calls, written once for both families: score_all.hip (ComplEx / DistMult: the block is one matrix
// product, mkb_all_*) and score_all_dist.hip (TransE / RotatE / pRotatE: the block is a sum of distances, mkb_dist_all_*).  The
// families differ in the backward of the block and in what of the workspace that backward needs; the workspace plan, the entry
// checks, the model dispatch, the step and the six entry bodies are here, and each extern "C" symbol is a wrapper of one line.
// A family F is a struct of statics that its .hip file defines next to its kernels:
//   static constexpr bool covers(int model)        the models its calls take (the others: MKB_ERR_UNSUPPORTED with F::refusal)
//   static constexpr const char *refusal, *mode_text
//   struct Launch                                  its own launch fields of the plan (AllPlan<F>::launch)
//   static FamilyBytes plan(tb, B, Launch &)       fills them; the bytes of its partial buffer and of its tail behind the loss scratch
//   static void finish_block(S, B, N, ld, c0, c1, st)   S = c0 + c1 S where the forward's route left raw pair sums
//   template <int MODEL, bool HEAD> static int bwd(tb, gr, sample, B, dS, ld, gathered, P, w, st)
//                                                  dS [B, ld] -> the gradients (accumulated); w.Q holds the batch's queries.  gathered: dS
//                                                  is the forward's padded block, its pad columns exactly 0, and w.ids the forward's id list
#pragma once
#include "all_chain.h"
#include "rank_all.h"

#include <algorithm>

namespace mkb {

struct FamilyBytes {
    size_t part, tail;
};

// ---- workspace: Q [B, De], the score block [B, Npad] (which becomes dS), the id list [Npad], dQ [B, De], the stash [B, De] of
// all_stash_kernel, the family's partial buffer, the sort's storage, the loss scratch [1 + B], the family's tail
template <class F>
struct AllPlan {
    PairSortPlan sort;
    typename F::Launch launch;
    size_t s_off, ids_off, dq_off, stash_off, part_off, sort_off, scr_off, tail_off, total;
};
struct AllWs {
    float *Q, *S;
    int64_t *ids;
    float *dQ, *stash, *part;
    void *sort;
    float *scratch, *tail;
};

// The shapes one int32 sort, one int32 GEMM and the softmax's B * ld limit cover (B >= 1 is the caller's).  false: outside them, or
// the sort's size query failed (*rc < 0)
template <class F>
static bool all_plan(const mkb_tables_t *tb, int64_t B, AllPlan<F> &P, int *rc) {
    *rc = 0;
    const int64_t N = tb->n_entity, Npad = all_npad(N), De = tb->entity_dim;
    if (N <= 0 || tb->n_relation <= 0 || De <= 0 || Npad >= (1 << 30) || N + tb->n_relation > INT32_MAX || B > INT32_MAX / 2 ||
        B * Npad > INT32_MAX || B * De > INT32_MAX)
        return false;
    if ((*rc = pair_sort_plan(N + tb->n_relation, 2 * B, P.sort))) return false;
    const FamilyBytes fam = F::plan(tb, B, P.launch);
    P.s_off = up256((size_t)B * De * 4);
    P.ids_off = P.s_off + up256((size_t)B * Npad * 4);
    P.dq_off = P.ids_off + up256((size_t)Npad * 8);
    P.stash_off = P.dq_off + up256((size_t)B * De * 4);
    P.part_off = P.stash_off + up256((size_t)B * De * 4);
    P.sort_off = P.part_off + up256(fam.part);
    P.scr_off = P.sort_off + P.sort.total;
    P.tail_off = P.scr_off + up256((size_t)(B + 1) * 4);
    P.total = P.tail_off + up256(fam.tail);
    return true;
}

template <class F>
static AllWs all_carve(const AllPlan<F> &P, void *ws) {
    unsigned char *b = (unsigned char *)ws;
    return AllWs{(float *)b, (float *)(b + P.s_off), (int64_t *)(b + P.ids_off), (float *)(b + P.dq_off), (float *)(b + P.stash_off),
                 (float *)(b + P.part_off), b + P.sort_off, (float *)(b + P.scr_off), (float *)(b + P.tail_off)};
}

// dispatch_model_side (common.h) over the family's models; the others are refused and no kernel is instantiated for them
template <class F, class Fn>
static int all_dispatch(int model, bool head, Fn &&f) {
    if (!F::covers(model)) return set_error(MKB_ERR_UNSUPPORTED, "%s", F::refusal);
    return dispatch_model_side(model, head, [&](auto m, auto h) {
        if constexpr (F::covers(decltype(m)::value)) return f(m, h);
        else return (int)MKB_ERR_UNSUPPORTED;
    });
}

// what every entry point that takes tables, a batch and the workspace checks, in this order
template <class F>
static int all_check(const mkb_tables_t *tb, const int64_t *sample, int64_t B, int mode, const void *ws, int64_t ws_bytes, AllPlan<F> &P) {
    if (int rc = validate_tables(tb)) return rc;
    MKB_REQUIRE(sample && ws, "null pointer");
    MKB_REQUIRE(mode == MKB_MODE_HEAD || mode == MKB_MODE_TAIL, "%s", F::mode_text);
    MKB_REQUIRE(B >= 1, "B must be >= 1");
    if (!F::covers(tb->model)) return set_error(MKB_ERR_UNSUPPORTED, "%s", F::refusal);
    MKB_REQUIRE(tb->entity_dim <= 4 * kWGr, "rows of more than 4096 units are not supported");
    int rc;
    if (!all_plan(tb, B, P, &rc)) {
        if (rc) return rc;
        MKB_REQUIRE(false, "B * (n_entity + 3) and B * entity_dim must stay below 2^31, n_entity below 2^30");
    }
    MKB_REQUIRE(ws_bytes >= (int64_t)P.total && (((uintptr_t)ws) & 255) == 0, "workspace too small / unaligned");
    return MKB_OK;
}

// The step behind the three *_step calls of a family, whose checks (all_check among them) have passed: the forward block, finished
// where the route left raw pair sums, the loss on it -- loss(S, ld, scratch) launches it and leaves dS in S --, the backward.
template <class F, class Loss>
static int all_step(const mkb_tables_t *tb, const mkb_grads_t *gr, const int64_t *sample, int64_t B, int mode, const AllPlan<F> &P,
                    void *ws, hipStream_t st, Loss &&loss) {
    const AllWs w = all_carve(P, ws);
    const int64_t N = tb->n_entity;
    int64_t ld_S = 0;
    auto finish = [&](float c0, float c1, int64_t ld) {
        ld_S = ld;
        if (!(c0 == 0.f && c1 == 1.f)) F::finish_block(w.S, B, N, ld, c0, c1, st);
        loss(w.S, ld, w.scratch);
    };
    return all_dispatch<F>(tb->model, mode == MKB_MODE_HEAD, [&](auto m, auto h) {
        if (int rc = run_rank<m(), h()>(tb, sample, B, w.Q, w.S, w.ids, st, finish)) return rc;
        return F::template bwd<m(), h()>(tb, gr, sample, B, w.S, ld_S, ld_S > N, P, w, st);
    });
}

// ---- the six entry bodies: mkb_all_X and mkb_dist_all_X are all_X<their family>
template <class F>
static int64_t all_workspace_bytes(const mkb_tables_t *tb, int64_t B) {
    AllPlan<F> P;
    int rc;
    if (!tb || B <= 0 || !F::covers(tb->model) || !all_plan(tb, B, P, &rc)) return 0;
    return (int64_t)P.total;
}

template <class F>
static int all_score_fwd(const mkb_tables_t *tb, const int64_t *sample, int64_t B, int mode, float *scores, void *ws, int64_t ws_bytes,
                         void *stream) {
    AllPlan<F> P;
    MKB_REQUIRE(scores, "null pointer");
    if (int rc = all_check(tb, sample, B, mode, ws, ws_bytes, P)) return rc;
    const AllWs w = all_carve(P, ws);
    hipStream_t st = (hipStream_t)stream;
    auto finish = [&](float f0, float f1, int64_t ld) {  // the evaluation's export: the bits mkb_rank_scores hands out
        hipLaunchKernelGGL(export_scores_kernel, dim3((unsigned)std::min<int64_t>((tb->n_entity + 255) / 256, 64), (unsigned)B), dim3(256), 0,
                           st, w.S, scores, tb->n_entity, ld, f0, f1);
    };
    return all_dispatch<F>(tb->model, mode == MKB_MODE_HEAD,
                           [&](auto m, auto h) { return run_rank<m(), h()>(tb, sample, B, w.Q, w.S, w.ids, st, finish); });
}

template <class F>
static int all_score_bwd(const mkb_tables_t *tb, const mkb_grads_t *gr, const int64_t *sample, int64_t B, int mode, const float *dscore,
                         int64_t ld, void *ws, int64_t ws_bytes, void *stream) {
    AllPlan<F> P;
    MKB_REQUIRE(gr && gr->g_ent && gr->g_rel && dscore, "null pointer");
    if (int rc = all_check(tb, sample, B, mode, ws, ws_bytes, P)) return rc;
    MKB_REQUIRE(ld >= tb->n_entity && B * ld <= INT32_MAX, "need ld >= n_entity and B * ld below 2^31");
    const AllWs w = all_carve(P, ws);
    hipStream_t st = (hipStream_t)stream;
    return all_dispatch<F>(tb->model, mode == MKB_MODE_HEAD, [&](auto m, auto h) {
        const RowArgs ra = query_build_args(tb->ent, tb->rel, sample, w.Q, tb->entity_dim, tb->relation_dim, tb->hidden_dim, B, tb->phase_div);
        hipLaunchKernelGGL((query_build_kernel<m(), h()>), dim3((unsigned)B), dim3(256), 0, st, ra);
        return F::template bwd<m(), h()>(tb, gr, sample, B, dscore, ld, false, P, w, st);
    });
}

template <class F>
static int all_softmax_step(const mkb_tables_t *tb, const mkb_grads_t *gr, const int64_t *sample, const float *weight, int64_t B, int mode,
                            float temperature, const float *weight_sum, float *loss, float *pos, void *ws, int64_t ws_bytes, void *stream) {
    AllPlan<F> P;
    MKB_REQUIRE(gr && gr->g_ent && gr->g_rel && loss && pos, "null pointer");
    MKB_REQUIRE(temperature - temperature == 0.f && temperature > 0.f, "the softmax temperature must be finite and > 0");
    if (int rc = all_check(tb, sample, B, mode, ws, ws_bytes, P)) return rc;
    hipStream_t st = (hipStream_t)stream;
    return all_step(tb, gr, sample, B, mode, P, ws, st, [&](float *S, int64_t ld, float *scratch) {
        all_softmax_launch(S, B, tb->n_entity, ld, sample + (mode == MKB_MODE_HEAD ? 0 : 2), 3, weight, weight_sum, temperature, loss, pos,
                           scratch, st);
    });
}

template <class F>
static int all_kvs_step(const mkb_tables_t *tb, const mkb_grads_t *gr, const int64_t *sample, const float *weight, int64_t B, int mode,
                        const int64_t *keys, int64_t n_keys, float smoothing, int sum_over_entities, const float *weight_sum, float *loss,
                        float *pos, void *ws, int64_t ws_bytes, void *stream) {
    AllPlan<F> P;
    MKB_REQUIRE(gr && gr->g_ent && gr->g_rel && loss && pos, "null pointer");
    if (int rc = all_check(tb, sample, B, mode, ws, ws_bytes, P)) return rc;
    if (int rc = bce_check(tb->n_entity, tb->n_relation, mode, keys, n_keys, smoothing)) return rc;
    hipStream_t st = (hipStream_t)stream;
    return all_step(tb, gr, sample, B, mode, P, ws, st, [&](float *S, int64_t ld, float *scratch) {
        all_bce_launch(S, B, tb->n_entity, ld, sample, mode == MKB_MODE_HEAD, tb->n_relation, keys, n_keys, weight, weight_sum, smoothing,
                       sum_over_entities != 0, loss, pos, scratch, st);
    });
}

template <class F>
static int all_filtered_step(const mkb_tables_t *tb, const mkb_grads_t *gr, const int64_t *sample, const float *weight, int64_t B, int mode,
                             const int64_t *keys, int64_t n_keys, float T, float smoothing, const float *weight_sum, float *loss,
                             float *pos, void *ws, int64_t ws_bytes, void *stream) {
    AllPlan<F> P;
    MKB_REQUIRE(gr && gr->g_ent && gr->g_rel && loss && pos, "null pointer");
    MKB_REQUIRE(T - T == 0.f && T > 0.f, "the softmax temperature must be finite and > 0");
    if (int rc = all_check(tb, sample, B, mode, ws, ws_bytes, P)) return rc;
    if (int rc = bce_check(tb->n_entity, tb->n_relation, mode, keys, n_keys, smoothing, "filtered 1vsAll")) return rc;
    hipStream_t st = (hipStream_t)stream;
    return all_step(tb, gr, sample, B, mode, P, ws, st, [&](float *S, int64_t ld, float *scratch) {
        all_softmax_filtered_launch(S, B, tb->n_entity, ld, sample + (mode == MKB_MODE_HEAD ? 0 : 2), 3, sample, mode == MKB_MODE_HEAD,
                                    tb->n_relation, keys, n_keys, weight, weight_sum, T, smoothing, loss, pos, scratch, st);
    });
}

}  // namespace mkb
