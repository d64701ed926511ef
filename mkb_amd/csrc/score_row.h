// The general path (explicit candidate ids), each piece written once.  The table view its kernels take; the lane-strided sum of
// the pair terms of one staged query against one candidate row (forward); one unit of one pair's gradient and the walk over a
// chunk of the candidate-sorted pair list (backward).  Users: score_general.hip (a row's K candidates: forward, both backward
// passes), score_relation.hip (the relations of an (h, ?, t) query and the slot forward: pair_row_sum, table_row), score_cand.hip
// (the slot backward), pair_sort.hip (table_row).  Every forward finishes with wave_sum and finish_score, so that the same
// (h, r, t) gives the same bits on any of them.
#pragma once
#include "common.h"
#include "query_side.h"

namespace mkb {

struct TablesDev {
    const float *ent, *rel, *modulus;
    int64_t De, Dr;
    int d;
    float gamma, kd;
    int vec4;  // rows (and their complex halves) are 16-byte aligned and a multiple of 4 units long
};

static inline TablesDev to_dev(const mkb_tables_t *tb) {
    TablesDev t;
    t.ent = tb->ent; t.rel = tb->rel; t.modulus = tb->modulus;
    t.De = tb->entity_dim; t.Dr = tb->relation_dim; t.d = tb->hidden_dim;
    t.gamma = tb->gamma; t.kd = tb->phase_div;
    const bool cp = tb->model == MKB_ROTATE;
    t.vec4 = ((((uintptr_t)tb->ent) & 15) == 0 && tb->entity_dim % 4 == 0 && (!cp || tb->hidden_dim % 4 == 0)) ? 1 : 0;
    return t;
}

#ifdef __HIPCC__
// An id as a row of its table: one outside it reads as the nearest row (the glue flags it, mkb_check_ids), nothing out of bounds.
__device__ __forceinline__ int64_t table_row(int64_t id, int64_t n) { return id < 0 ? 0 : (id < n ? id : n - 1); }

// This lane's share of sum_k pair(q[k], x[k]): q is the query staged in LDS (16-byte aligned; complex-query models: re at k, im at
// d + k), x the candidate's entity row.  vec4: 16-byte loads of both, four terms grouped (a + b) + (c + d) per step of 256 units;
// otherwise one unit per step of 64.  The caller adds the lanes up (wave_sum).
template <int MODEL, bool HEAD>
__device__ __forceinline__ float pair_row_sum(const TablesDev &T, const float *q_lds, const float *x, int lane, bool vec4) {
    float acc = 0.f;
    if constexpr (ModelTraits<MODEL>::cplx_pair) {
        if (vec4) {  // 16-byte loads of the candidate row halves and of the staged query
            for (int k = lane * 4; k < T.d; k += 256) {
                const float4 xr = *reinterpret_cast<const float4 *>(x + k), xi = *reinterpret_cast<const float4 *>(x + T.d + k);
                const float4 qr = *reinterpret_cast<const float4 *>(q_lds + k), qi = *reinterpret_cast<const float4 *>(q_lds + T.d + k);
                const f2 t0 = pair_term_cmod2(f2{qr.x, qr.y}, f2{qi.x, qi.y}, f2{xr.x, xr.y}, f2{xi.x, xi.y});
                const f2 t1 = pair_term_cmod2(f2{qr.z, qr.w}, f2{qi.z, qi.w}, f2{xr.z, xr.w}, f2{xi.z, xi.w});
                acc += (t0.x + t0.y) + (t1.x + t1.y);
            }
        } else {
            for (int k = lane; k < T.d; k += 64)
                acc += pair_term_cmod(Cplx{q_lds[k], q_lds[T.d + k]}, Cplx{x[k], x[T.d + k]});
        }
    } else {
        if (vec4) {
            for (int k = lane * 4; k < (int)T.De; k += 256) {
                const float4 xv = *reinterpret_cast<const float4 *>(x + k), qv = *reinterpret_cast<const float4 *>(q_lds + k);
                acc += (pair_term_real<MODEL, HEAD>(qv.x, xv.x, T.kd) + pair_term_real<MODEL, HEAD>(qv.y, xv.y, T.kd))
                       + (pair_term_real<MODEL, HEAD>(qv.z, xv.z, T.kd) + pair_term_real<MODEL, HEAD>(qv.w, xv.w, T.kd));
            }
        } else {
            for (int k = lane; k < (int)T.De; k += 64) acc += pair_term_real<MODEL, HEAD>(q_lds[k], x[k], T.kd);
        }
    }
    return acc;
}

// One unit of one pair: the query unit q against the candidate unit x with the seed g -> the contributions to q and to x.  Real
// models use the .re halves (the .im come back 0).  extra += pRotatE's g * |sin z| (the modulus gradient), where the caller
// wants it.
template <int MODEL, bool HEAD>
__device__ __forceinline__ void pair_unit_bwd(Cplx q, Cplx x, float g, float kd, float modulus, Cplx &dq, Cplx &dx, float &extra) {
    float e0 = 0.f;
    if constexpr (ModelTraits<MODEL>::cplx_pair) {
        pair_bwd_cmod(q, x, g, dq, dx);
    } else if constexpr (ModelTraits<MODEL>::cplx_query) {  // ComplEx: a dot product over both halves
        pair_bwd_real<MODEL, HEAD>(q.re, x.re, g, kd, modulus, dq.re, dx.re, e0);
        pair_bwd_real<MODEL, HEAD>(q.im, x.im, g, kd, modulus, dq.im, dx.im, e0);
    } else {
        pair_bwd_real<MODEL, HEAD>(q.re, x.re, g, kd, modulus, dq.re, dx.re, e0);
        extra += g * e0;
        dq.im = dx.im = 0.f;
    }
}

// The walk over pairs lo .. hi - 1 of the candidate-sorted pair list for whatever a lane owns: the candidate's unit and its
// running gradient stay in the caller's registers and leave only when the candidate changes.  load(c): candidate c begins (load
// its unit, zero the running gradient); pair(p): add pair p's contribution; flush(c): candidate c's run is over.
constexpr int kChunkPairs = 64;  // pairs per workgroup of the kernels that walk
template <class Load, class Pair, class Flush>
__device__ __forceinline__ void walk_sorted_pairs(const int *__restrict__ sorted_cand, const int *__restrict__ sorted_pair, int lo, int hi,
                                                  Load &&load, Pair &&pair, Flush &&flush) {
    int cur = -1;
    auto end_run = [&]() {  // (an early return, not `if (cur >= 0)`: the RotatE and ComplEx walks then compile as they always have)
        if (cur < 0) return;
        flush(cur);
    };
    for (int p = lo; p < hi; ++p) {
        const int c = sorted_cand[p];  // (uniform across the workgroup; a row of the table: pair_sort.hip)
        if (c != cur) {
            end_run();
            cur = c;
            load(c);
        }
        pair(sorted_pair[p]);
    }
    end_run();
}
#endif

}  // namespace mkb
