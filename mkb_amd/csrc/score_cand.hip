// Candidate lists in any one slot of a triple, with a backward: mkb_cand_score_fwd / mkb_cand_score_bwd (what
// BaseModel.score_candidates and, on top of it, Distillation.distill score).
//
// Forward : head and relation part: the slot forward of score_relation.hip (launch_slot_scores, score_slot.h) with a list per
//           row.  Tail part: the general forward (mkb_score_fwd, tail mode).
// Backward: head and relation part, two passes, neither writes a gradient per pair.  Row pass: the gradients of the two fixed rows
//           accumulate in registers over the row's candidates (one atomic per element and row).  Candidate pass: the B*M pairs
//           radix-sorted by candidate (pair_sort.h), 64 consecutive pairs per workgroup, one atomic per element and run of equal
//           candidates (walk_sorted_pairs, score_row.h).  Tail part: the general two-pass backward (mkb_score_bwd, tail mode).
#include "common.h"
#include "pair_sort.h"
#include "query_side.h"
#include "score_row.h"
#include "score_slot.h"

namespace mkb {

// One unit of one pair from its rows: q = query(e, r) against x with the seed g -> the contributions to e, r and x.  Real models
// use the .re halves.  extra: as pair_unit_bwd's.
template <int MODEL>
__device__ __forceinline__ void slot_pair_bwd(Cplx e, Cplx r, Cplx x, float g, float kd, float modulus, Cplx &de, Cplx &dr, Cplx &dx,
                                              float &extra) {
    Cplx dq;
    if constexpr (ModelTraits<MODEL>::cplx_query) {
        pair_unit_bwd<MODEL, false>(query_of<MODEL, false>(e, r, kd), x, g, kd, modulus, dq, dx, extra);
        query_chain<MODEL, false>(e, r, dq, kd, de, dr);
    } else {
        pair_unit_bwd<MODEL, false>(Cplx{query_of<MODEL, false>(e.re, r.re, kd), 0.f}, x, g, kd, modulus, dq, dx, extra);
        query_chain<MODEL, false>(e.re, r.re, dq.re, kd, de.re, dr.re);
        de.im = dr.im = 0.f;
    }
}

// Row pass: one workgroup per row, lanes own units.  The units of the two fixed operands stay in registers, their gradients
// accumulate over the row's M candidates and leave as one atomic per element and row; nothing is written per pair.
template <int MODEL, bool VARY_HEAD>
__global__ __launch_bounds__(kSlotBlock) void slot_bwd_row_kernel(TablesDev T, mkb_grads_t G, const int64_t *__restrict__ sample,
                                                                  const int64_t *__restrict__ cand, int M, int64_t n_table,
                                                                  const float *__restrict__ dscore) {
    __shared__ float red[kSlotWaves];
    const int64_t i = blockIdx.x;
    const int64_t h = sample[3 * i], r = sample[3 * i + 1], t = sample[3 * i + 2];
    const float *ea = VARY_HEAD ? T.rel + r * T.Dr : T.ent + h * T.De, *et = T.ent + t * T.De;
    float *g_a = VARY_HEAD ? G.g_rel + r * T.Dr : G.g_ent + h * T.De, *g_t = G.g_ent + t * T.De;
    const int U = ModelTraits<MODEL>::cplx_query ? T.d : (int)T.De;
    const float modulus = (MODEL == MKB_PROTATE) ? T.modulus[0] : 0.f;
    const int64_t *list = cand + i * M;
    const float *seed = dscore + i * M;
    float extra = 0.f;
    for (int u = threadIdx.x; u < U; u += kSlotBlock) {
        const Cplx a = VARY_HEAD ? rel_unit<MODEL>(ea, T.d, u) : ent_unit<MODEL>(ea, T.d, u);
        const Cplx x = ent_unit<MODEL>(et, T.d, u);
        Cplx da{0.f, 0.f}, dt{0.f, 0.f};
        for (int j = 0; j < M; ++j) {
            const int64_t id = table_row(list[j], n_table);  // (uniform across the workgroup)
            Cplx de, dr, dx;
            if constexpr (VARY_HEAD) {
                slot_pair_bwd<MODEL>(ent_unit<MODEL>(T.ent + id * T.De, T.d, u), a, x, seed[j], T.kd, modulus, de, dr, dx, extra);
                da.re += dr.re; da.im += dr.im;
            } else {
                slot_pair_bwd<MODEL>(a, rel_unit<MODEL>(T.rel + id * T.Dr, T.d, u), x, seed[j], T.kd, modulus, de, dr, dx, extra);
                da.re += de.re; da.im += de.im;
            }
            dt.re += dx.re; dt.im += dx.im;
        }
        row_grad_atomic<MODEL, VARY_HEAD>(g_a, T.d, u, da);
        row_grad_atomic<MODEL, false>(g_t, T.d, u, dt);
    }
    if constexpr (MODEL == MKB_PROTATE) {  // d score / d modulus = - sum_k |sin z|: once per pair, so in this pass only
        extra = block_sum_4waves(extra, red);
        if (threadIdx.x == 0) atomicAdd(G.g_modulus, -extra);
    }
}

// Candidate pass: workgroup (x, y) = kChunkPairs consecutive pairs of the candidate-sorted pair list, units 256 y .. 256 y + 255.
// A lane keeps its unit of the candidate's row and the running gradient in registers and adds to the candidate's gradient row
// only when the candidate changes; the pair term is evaluated again from the pair's fixed rows.
template <int MODEL, bool VARY_HEAD>
__global__ __launch_bounds__(kSlotBlock) void slot_bwd_cand_kernel(TablesDev T, mkb_grads_t G, const int *__restrict__ sorted_cand,
                                                                   const int *__restrict__ sorted_pair, int n_pairs, int M,
                                                                   const int64_t *__restrict__ sample,
                                                                   const float *__restrict__ dscore) {
    const int lo = blockIdx.x * kChunkPairs, hi = min(n_pairs, lo + kChunkPairs);
    const int U = ModelTraits<MODEL>::cplx_query ? T.d : (int)T.De;
    const int u = blockIdx.y * kSlotBlock + threadIdx.x;
    if (u >= U) return;
    const float modulus = (MODEL == MKB_PROTATE) ? T.modulus[0] : 0.f;
    Cplx c{0.f, 0.f}, dc{0.f, 0.f};
    float unused = 0.f;
    walk_sorted_pairs(
        sorted_cand, sorted_pair, lo, hi,
        [&](int id) {
            c = VARY_HEAD ? ent_unit<MODEL>(T.ent + (int64_t)id * T.De, T.d, u) : rel_unit<MODEL>(T.rel + (int64_t)id * T.Dr, T.d, u);
            dc = Cplx{0.f, 0.f};
        },
        [&](int pair) {
            const int64_t i = pair / M;
            const Cplx x = ent_unit<MODEL>(T.ent + sample[3 * i + 2] * T.De, T.d, u);
            Cplx de, dr, dx;
            if constexpr (VARY_HEAD) {
                slot_pair_bwd<MODEL>(c, rel_unit<MODEL>(T.rel + sample[3 * i + 1] * T.Dr, T.d, u), x, dscore[pair], T.kd, modulus, de, dr, dx, unused);
                dc.re += de.re; dc.im += de.im;
            } else {
                slot_pair_bwd<MODEL>(ent_unit<MODEL>(T.ent + sample[3 * i] * T.De, T.d, u), c, x, dscore[pair], T.kd, modulus, de, dr, dx, unused);
                dc.re += dr.re; dc.im += dr.im;
            }
        },
        [&](int id) {
            if constexpr (VARY_HEAD) row_grad_atomic<MODEL, false>(G.g_ent + (int64_t)id * T.De, T.d, u, dc);
            else row_grad_atomic<MODEL, true>(G.g_rel + (int64_t)id * T.Dr, T.d, u, dc);
        });
}

static bool part_ok(int part) { return part >= MKB_PART_HEAD && part <= MKB_PART_TAIL; }
static bool shape_ok(const mkb_tables_t *tb, int64_t B, int64_t M) {
    return B >= 0 && B <= INT32_MAX && M >= 1 && M <= INT32_MAX && B * M <= INT32_MAX && tb->n_entity <= INT32_MAX
           && tb->n_relation <= INT32_MAX;
}
static int64_t cand_table_rows(const mkb_tables_t *tb, int part) { return part == MKB_PART_HEAD ? tb->n_entity : tb->n_relation; }

static int check_cand_call(const mkb_tables_t *tb, const int64_t *sample, const int64_t *cand, int64_t B, int64_t M, int part) {
    if (int rc = validate_tables(tb)) return rc;
    MKB_REQUIRE(sample != nullptr && cand != nullptr, "null pointer");
    MKB_REQUIRE(part_ok(part), "bad part %d", part);
    MKB_REQUIRE(shape_ok(tb, B, M), "B must lie in [0, 2^31 - 1], M in [1, 2^31 - 1], B * M and the tables' rows below 2^31");
    return slot_rows_check(tb);
}

template <int MODEL, bool VARY_HEAD>
static int launch_slot_bwd(const mkb_tables_t *tb, const mkb_grads_t &G, const int64_t *sample, const int64_t *cand, int64_t B, int M,
                           const float *dscore, void *ws, const PairSortPlan &plan, hipStream_t st) {
    const TablesDev T = to_dev(tb);
    const int64_t n = B * M, n_table = cand_table_rows(tb, VARY_HEAD ? MKB_PART_HEAD : MKB_PART_RELATION);
    const int *sorted_cand, *sorted_pair;
    if (int rc = pair_sort_launch(cand, n, n_table, ws, plan, st, &sorted_cand, &sorted_pair)) return rc;
    hipLaunchKernelGGL((slot_bwd_row_kernel<MODEL, VARY_HEAD>), dim3((unsigned)B), dim3(kSlotBlock), 0, st, T, G, sample, cand, M, n_table,
                       dscore);
    const int U = ModelTraits<MODEL>::cplx_query ? T.d : (int)T.De;
    const dim3 grid((unsigned)((n + kChunkPairs - 1) / kChunkPairs), (unsigned)((U + kSlotBlock - 1) / kSlotBlock));
    hipLaunchKernelGGL((slot_bwd_cand_kernel<MODEL, VARY_HEAD>), grid, dim3(kSlotBlock), 0, st, T, G, sorted_cand, sorted_pair, (int)n, M,
                       sample, dscore);
    MKB_LAUNCH_CHECK();
    return MKB_OK;
}

}  // namespace mkb

using namespace mkb;

extern "C" int mkb_cand_score_fwd(const mkb_tables_t *tb, const int64_t *sample, const int64_t *cand, int64_t B, int64_t M, int part,
                                  float *score, void *stream) {
    if (int rc = check_cand_call(tb, sample, cand, B, M, part)) return rc;
    MKB_REQUIRE(score != nullptr, "score is null");
    if (B == 0) return MKB_OK;
    if (part == MKB_PART_TAIL) return mkb_score_fwd(tb, sample, cand, B, M, MKB_MODE_TAIL, score, stream);  // default mode's instantiation
    if (int rc = launch_slot_scores(tb, sample, B, cand, M, M, part == MKB_PART_HEAD, score, M, (hipStream_t)stream)) return rc;
    MKB_LAUNCH_CHECK();
    return MKB_OK;
}

extern "C" int64_t mkb_cand_score_bwd_workspace_bytes(const mkb_tables_t *tb, int64_t B, int64_t M, int part) {
    if (!tb || B <= 0 || !part_ok(part) || !shape_ok(tb, B, M)) return 0;
    if (part == MKB_PART_TAIL) return mkb_score_bwd_workspace_bytes(tb, B, M, MKB_MODE_TAIL);
    PairSortPlan plan;
    return pair_sort_plan(cand_table_rows(tb, part), B * M, plan) ? -1 : (int64_t)plan.total;
}

extern "C" int mkb_cand_score_bwd(const mkb_tables_t *tb, const mkb_grads_t *gr, const int64_t *sample, const int64_t *cand, int64_t B,
                                  int64_t M, int part, const float *dscore, void *ws, int64_t ws_bytes, void *stream) {
    if (int rc = check_cand_call(tb, sample, cand, B, M, part)) return rc;
    MKB_REQUIRE(gr && gr->g_ent && gr->g_rel && dscore, "null gradient buffer");
    MKB_REQUIRE(tb->model != MKB_PROTATE || gr->g_modulus, "pRotatE needs g_modulus");
    if (B == 0) return MKB_OK;
    const int64_t need = mkb_cand_score_bwd_workspace_bytes(tb, B, M, part);
    if (need < 0) return MKB_ERR_HIP;  // (the sort's size query failed: its message stands)
    MKB_REQUIRE(need == 0 || (ws != nullptr && (((uintptr_t)ws) & 255) == 0 && ws_bytes >= need), "workspace null, too small or unaligned");
    if (part == MKB_PART_TAIL) return mkb_score_bwd(tb, gr, sample, cand, B, M, MKB_MODE_TAIL, dscore, ws, stream);
    PairSortPlan plan;
    if (int rc = pair_sort_plan(cand_table_rows(tb, part), B * M, plan)) return rc;
    return dispatch_model_side(tb->model, part == MKB_PART_HEAD, [&](auto m, auto vh) {
        return launch_slot_bwd<m(), vh()>(tb, *gr, sample, cand, B, (int)M, dscore, ws, plan, (hipStream_t)stream);
    });
}
