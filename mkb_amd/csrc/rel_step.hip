// Relation prediction as an auxiliary training term (include/mkb_hip.h, "relation prediction"): next to the entity losses a batch
// also minimises -log P(r | h, t) over ALL relations (Chen et al., AKBC 2021), weighted by lambda,
//     S_ij = score(h_i, j, t_i),   row_i = logsumexp_j (S_ij / T) - S_{i, r_i} / T,   value = lambda sum_i w_i row_i / W,
//     dS_ij = lambda (w_i / (W T)) (p_ij - [j = r_i]).
// mkb_rel_step is value and gradient in one call, mkb_rel_score_bwd the backward of the mkb_rel_scores block alone.
//
//   forward   the slot forward of score_relation.hip (launch_slot_scores) into the workspace block [B, n_relation]: every S_ij has
//             the bits of mkb_rel_scores, so pos[i] = S_{i, r_i} has the bits of mkb_score_fwd.
//   loss      all_softmax_launch (score_all.hip, untouched) on that block with target = sample + 1, stride 3.  lambda is a scale
//             on what the softmax leaves: rel_scale_kernel multiplies the value once, and both backward passes read a seed as
//             lambda dS_ij, so the value and every gradient element carry lambda exactly once -- and the explicit sequence
//             (mkb_rel_scores, mkb_all_softmax, lambda times its seeds into mkb_rel_score_bwd) gives the bits of this call.
//   backward  of the block, the pair terms recomputed in both passes (slot_pair_bwd's composition of model_math.h / query_side.h);
//             nothing of size [B, R, De] exists.
//       rel_bwd_pair_kernel  pair-major.  A workgroup owns sample row i and 256 units of it, one per lane; the lane's units of h_i and
//                            t_i stay in registers and their gradients accumulate over the R relation rows in order, eight
//                            relations' loads in flight per turn.  dH[i] and dT[i] leave with plain stores into the workspace
//                            [2, B, De]; pRotatE: the workgroup's sum_j dS_ij sum_k |sin z| into modpart [B, unit slices].
//       rel_bwd_rel_kernel   relation-major.  A workgroup owns kRelTile relations x 256 units and walks a slice of the batch rows in
//                            order: a lane holds its unit of the tile's relations and their sums in registers and loads the units
//                            of h_i and t_i once per tile, four rows' loads in flight.  The sums leave as one partial per slice,
//                            [slices, R, Dr]; rel_part_reduce_kernel adds them left to right and adds the total to g_rel once.
//                            With few relation tiles (WN18RR has 11 relations) the slices are what fills the device.
//       rel_ent_rows_kernel  the 2 B occurrences (heads, then tails) radix-sorted by entity (pair_sort.h); one workgroup per distinct
//                            entity sums its occurrences' dH / dT rows in sorted order -- the sort is stable: batch order, heads
//                            first -- and adds the sum to the g_ent row once.  Entities outside the batch are not touched.
//       rel_mod_kernel       pRotatE: the rows' partials summed in fixed order, added to g_modulus once.
// No float atomics: every gradient element has one writer and every sum a fixed order, so two runs give the same bits and a
// gradient buffer that held something ends as that + the term's gradient.
// One generic path serves the five models.  For ComplEx / DistMult the block is a matrix product (u = h o conj t, S = U R^T) that
// gemm_plan.h could take; that route has not been measured ahead of this one and is not taken.
#include "common.h"
#include "all_chain.h"  // all_softmax_launch, softmax_check, up256 (pair_sort.h, query_side.h)
#include "loss_math.h"
#include "score_row.h"
#include "score_slot.h"

#include <algorithm>

namespace mkb {

constexpr int kRelTile = 8;             // relations per workgroup of the relation-major pass: 16 + 16 registers per lane for ComplEx
constexpr int kRelRows = 4;             // batch rows whose loads the relation-major pass keeps in flight
constexpr int kPairTurn = 8;            // relations whose loads the pair-major pass keeps in flight
constexpr int kRelGroupsWanted = 2048;  // workgroups the relation-major pass aims for when it slices the batch
constexpr int kRelSliceRowsMin = 8;     // ... and the fewest batch rows a slice is worth

// One unit of one pair from its rows (score_cand.hip's slot_pair_bwd): q = query(e, r) against x with the seed g -> the
// contributions to e, r and x.  Real models use the .re halves.  extra += g |sin z| (pRotatE).
template <int MODEL>
__device__ __forceinline__ void rel_pair_bwd(Cplx e, Cplx r, Cplx x, float g, float kd, float modulus, Cplx &de, Cplx &dr, Cplx &dx,
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

struct RelBwdArgs {
    const float *ent, *rel, *modulus;
    const int64_t *sample;
    const float *dS;  // [B, ld]
    float *dHT;       // [2, B, De]
    float *modpart;   // [B, unit slices]
    float *part;      // [slices, R, Dr]
    int64_t De, Dr, ld;
    int d, U, B, R, rows;  // rows: batch rows per slice of the relation-major pass
    float kd, scale;       // scale: a seed is scale * dS_ij (lambda; 1 for a caller's seeds)
};

// value = lambda * the softmax's loss
static __global__ void rel_scale_kernel(float *__restrict__ loss, float lambda) {
    if (threadIdx.x == 0) loss[0] *= lambda;
}

// grid (B, ceil(U / 256)): one unit per lane.  (A lane that walked its row's units one after the other -- grid (B), a turn of 4 --
// waited for one L2 round trip per turn and unit: 240 of them in a row at hidden 1000, and the pass took what one workgroup took.)
template <int MODEL>
__global__ __launch_bounds__(256) void rel_bwd_pair_kernel(RelBwdArgs A) {
    constexpr bool CQ = ModelTraits<MODEL>::cplx_query;
    __shared__ float red[4];
    const int64_t i = blockIdx.x;
    const float *eh = A.ent + A.sample[3 * i] * A.De, *et = A.ent + A.sample[3 * i + 2] * A.De;
    const float *seed = A.dS + i * A.ld;
    float *dh = A.dHT + i * A.De, *dt = A.dHT + ((int64_t)A.B + i) * A.De;
    const float modulus = (MODEL == MKB_PROTATE) ? A.modulus[0] : 0.f;
    float extra = 0.f;
    const int u = blockIdx.y * 256 + threadIdx.x;
    if (u < A.U) {
        const Cplx a = ent_unit<MODEL>(eh, A.d, u), x = ent_unit<MODEL>(et, A.d, u);
        Cplx da{0.f, 0.f}, dx{0.f, 0.f};
        for (int j0 = 0; j0 < A.R; j0 += kPairTurn) {  // a turn: kPairTurn relations' units in flight (past the last: the last one again, not used)
            Cplx r[kPairTurn];
#pragma unroll
            for (int w = 0; w < kPairTurn; ++w) r[w] = rel_unit<MODEL>(A.rel + (int64_t)min(j0 + w, A.R - 1) * A.Dr, A.d, u);
#pragma unroll
            for (int w = 0; w < kPairTurn; ++w)
                if (j0 + w < A.R) {  // (uniform)
                    Cplx de, dr, dxx;
                    rel_pair_bwd<MODEL>(a, r[w], x, A.scale * seed[j0 + w], A.kd, modulus, de, dr, dxx, extra);
                    da.re += de.re; dx.re += dxx.re;
                    if constexpr (CQ) { da.im += de.im; dx.im += dxx.im; }
                }
        }
        dh[u] = da.re; dt[u] = dx.re;
        if constexpr (CQ) { dh[A.d + u] = da.im; dt[A.d + u] = dx.im; }
    }
    if constexpr (MODEL == MKB_PROTATE) {  // one partial per (row, unit slice): [B, gridDim.y]
        extra = block_sum_4waves(extra, red);
        if (threadIdx.x == 0) A.modpart[i * gridDim.y + blockIdx.y] = extra;
    }
}

// grid (ceil(R / kRelTile), ceil(U / 256), slices)
template <int MODEL>
__global__ __launch_bounds__(256) void rel_bwd_rel_kernel(RelBwdArgs A) {
    constexpr bool REL_IM = MODEL == MKB_COMPLEX;
    const int u = blockIdx.y * 256 + threadIdx.x;
    if (u >= A.U) return;  // (no barrier below)
    const int j0 = blockIdx.x * kRelTile;
    const float modulus = (MODEL == MKB_PROTATE) ? A.modulus[0] : 0.f;
    Cplx r[kRelTile], acc[kRelTile];
#pragma unroll
    for (int w = 0; w < kRelTile; ++w) {
        r[w] = rel_unit<MODEL>(A.rel + (int64_t)min(j0 + w, A.R - 1) * A.Dr, A.d, u);
        acc[w] = Cplx{0.f, 0.f};
    }
    const int i_lo = blockIdx.z * A.rows, i_hi = min(A.B, i_lo + A.rows);
    float unused = 0.f;
    auto row = [&](int i, Cplx a, Cplx x) {
        const float *seed = A.dS + (int64_t)i * A.ld + j0;
#pragma unroll
        for (int w = 0; w < kRelTile; ++w)
            if (j0 + w < A.R) {  // (uniform)
                Cplx de, dr, dx;
                rel_pair_bwd<MODEL>(a, r[w], x, A.scale * seed[w], A.kd, modulus, de, dr, dx, unused);
                acc[w].re += dr.re;
                if constexpr (REL_IM) acc[w].im += dr.im;
            }
    };
    for (int i = i_lo; i < i_hi; i += kRelRows) {  // kRelRows rows' loads in flight (past the last: the last one again, not used); added in batch order
        Cplx a[kRelRows], x[kRelRows];
#pragma unroll
        for (int k = 0; k < kRelRows; ++k) {
            const int64_t ik = min(i + k, i_hi - 1);
            a[k] = ent_unit<MODEL>(A.ent + A.sample[3 * ik] * A.De, A.d, u);
            x[k] = ent_unit<MODEL>(A.ent + A.sample[3 * ik + 2] * A.De, A.d, u);
        }
#pragma unroll
        for (int k = 0; k < kRelRows; ++k)
            if (i + k < i_hi) row(i + k, a[k], x[k]);  // (uniform)
    }
    float *out = A.part + (int64_t)blockIdx.z * A.R * A.Dr;
#pragma unroll
    for (int w = 0; w < kRelTile; ++w)
        if (j0 + w < A.R) {
            float *o = out + (int64_t)(j0 + w) * A.Dr;
            o[u] = acc[w].re;
            if constexpr (REL_IM) o[A.d + u] = acc[w].im;
        }
}

// g_rel[k] += part[0][k] + part[1][k] + ... left to right
static __global__ __launch_bounds__(256) void rel_part_reduce_kernel(const float *__restrict__ part, float *__restrict__ g_rel, int64_t n,
                                                                     int slices) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    float acc = part[k];
    for (int z = 1; z < slices; ++z) acc += part[(int64_t)z * n + k];
    g_rel[k] += acc;
}

// One workgroup per sorted position of the 2 B occurrences; the position that opens a run of equal entities owns the row.
// vals: the occurrence, which is its row of dHT [2 B, De].
static __global__ __launch_bounds__(256) void rel_ent_rows_kernel(const int *__restrict__ keys, const int *__restrict__ vals, int n,
                                                                  const float *__restrict__ dHT, int64_t De, float *__restrict__ g_ent) {
    const int pos = blockIdx.x;
    const int key = keys[pos];
    if (pos > 0 && keys[pos - 1] == key) return;  // (uniform)
    float *g = g_ent + (int64_t)key * De;
    for (int64_t k = threadIdx.x; k < De; k += 256) {
        float acc = 0.f;
        for (int j = pos; j < n && keys[j] == key; ++j) acc += dHT[(int64_t)vals[j] * De + k];
        g[k] += acc;
    }
}

// g_modulus[0] -= sum of the n partials: lane-strided partial sums, then the fixed tree
static __global__ __launch_bounds__(256) void rel_mod_kernel(const float *__restrict__ modpart, int n, float *__restrict__ g_modulus) {
    __shared__ float red[4];
    float acc = 0.f;
    for (int i = threadIdx.x; i < n; i += 256) acc += modpart[i];
    acc = block_sum_256(acc, red);
    if (threadIdx.x == 0) g_modulus[0] += -acc;
}

// ---- workspace: the block [B, R] (which becomes dS), dHT [2, B, De], modpart [B, unit slices], the relation partials [slices, R, Dr], the
// sort's storage, the loss scratch [1 + B]
struct RelPlan {
    PairSortPlan sort;
    int slices, rows;
    size_t ht_off, mod_off, part_off, sort_off, scr_off, total;
};

// The shapes one int32 sort and the softmax's B * ld limit cover (B >= 1 is the caller's).  false: outside them, or the sort's
// size query failed (*rc < 0)
static bool rel_plan(const mkb_tables_t *tb, int64_t B, RelPlan &P, int *rc) {
    *rc = 0;
    const int64_t N = tb->n_entity, R = tb->n_relation, De = tb->entity_dim, Dr = tb->relation_dim;
    if (N <= 0 || R <= 0 || De <= 0 || Dr <= 0 || N > INT32_MAX || B > INT32_MAX / 2 || B * R > INT32_MAX || B * De > INT32_MAX / 2 ||
        R * Dr > INT32_MAX)
        return false;
    if ((*rc = pair_sort_plan(N, 2 * B, P.sort))) return false;
    const int U = (tb->model == MKB_ROTATE || tb->model == MKB_COMPLEX) ? tb->hidden_dim : (int)De;
    const int64_t tiles = ((R + kRelTile - 1) / kRelTile) * ((U + 255) / 256);
    const int64_t wanted = std::min<int64_t>((kRelGroupsWanted + tiles - 1) / tiles, (B + kRelSliceRowsMin - 1) / kRelSliceRowsMin);
    P.rows = (int)((B + wanted - 1) / std::max<int64_t>(wanted, 1));
    P.slices = (int)((B + P.rows - 1) / P.rows);
    P.ht_off = up256((size_t)B * R * 4);
    P.mod_off = P.ht_off + up256((size_t)2 * B * De * 4);
    P.part_off = P.mod_off + up256((size_t)B * ((U + 255) / 256) * 4);
    P.sort_off = P.part_off + up256((size_t)P.slices * R * Dr * 4);
    P.scr_off = P.sort_off + P.sort.total;
    P.total = P.scr_off + up256((size_t)(B + 1) * 4);
    return true;
}

// what the two calls that take a workspace check, in this order, before any launch (B >= 1)
static int rel_check(const mkb_tables_t *tb, int64_t B, const void *ws, int64_t ws_bytes, RelPlan &P) {
    int rc;
    if (!rel_plan(tb, B, P, &rc)) {
        if (rc) return rc;
        MKB_REQUIRE(false, "B * n_relation, 2 * B * entity_dim, n_relation * relation_dim and n_entity must stay below 2^31");
    }
    MKB_REQUIRE(ws != nullptr && (((uintptr_t)ws) & 255) == 0 && ws_bytes >= (int64_t)P.total, "workspace null, too small or unaligned");
    return MKB_OK;
}

// dS [B, ld] -> the gradients, added to gr
template <int MODEL>
static int rel_bwd(const mkb_tables_t *tb, const mkb_grads_t *gr, const int64_t *sample, int64_t B, const float *dS, int64_t ld,
                   float scale, const RelPlan &P, void *ws, hipStream_t st) {
    unsigned char *b = (unsigned char *)ws;
    RelBwdArgs A{};
    A.ent = tb->ent; A.rel = tb->rel; A.modulus = tb->modulus; A.sample = sample; A.dS = dS;
    A.dHT = (float *)(b + P.ht_off); A.modpart = (float *)(b + P.mod_off); A.part = (float *)(b + P.part_off);
    A.De = tb->entity_dim; A.Dr = tb->relation_dim; A.ld = ld; A.d = tb->hidden_dim;
    A.U = ModelTraits<MODEL>::cplx_query ? tb->hidden_dim : (int)tb->entity_dim;
    A.B = (int)B; A.R = (int)tb->n_relation; A.rows = P.rows; A.kd = tb->phase_div; A.scale = scale;
    PairKeySegs segs{};
    segs.seg[0] = PairKeySeg{sample, 3, B, tb->n_entity, 0};      // the heads
    segs.seg[1] = PairKeySeg{sample + 2, 3, B, tb->n_entity, 0};  // the tails
    segs.n_segs = 2;
    const int *keys, *vals;
    if (int rc = pair_sort_launch_segs(segs, b + P.sort_off, P.sort, st, &keys, &vals)) return rc;
    const unsigned uslices = (unsigned)((A.U + 255) / 256);
    hipLaunchKernelGGL((rel_bwd_pair_kernel<MODEL>), dim3((unsigned)B, uslices), dim3(256), 0, st, A);
    const dim3 grid((unsigned)((A.R + kRelTile - 1) / kRelTile), uslices, (unsigned)P.slices);
    hipLaunchKernelGGL((rel_bwd_rel_kernel<MODEL>), grid, dim3(256), 0, st, A);
    const int64_t n_rel = (int64_t)A.R * A.Dr;
    hipLaunchKernelGGL(rel_part_reduce_kernel, dim3((unsigned)((n_rel + 255) / 256)), dim3(256), 0, st, A.part, gr->g_rel, n_rel, P.slices);
    hipLaunchKernelGGL(rel_ent_rows_kernel, dim3((unsigned)(2 * B)), dim3(256), 0, st, keys, vals, (int)(2 * B), A.dHT, A.De, gr->g_ent);
    if constexpr (MODEL == MKB_PROTATE)
        hipLaunchKernelGGL(rel_mod_kernel, dim3(1), dim3(256), 0, st, A.modpart, (int)(B * uslices), gr->g_modulus);
    MKB_LAUNCH_CHECK();
    return MKB_OK;
}

static int rel_bwd_dispatch(const mkb_tables_t *tb, const mkb_grads_t *gr, const int64_t *sample, int64_t B, const float *dS, int64_t ld,
                            float scale, const RelPlan &P, void *ws, hipStream_t st) {
    return dispatch_model_side(tb->model, false, [&](auto m, auto) { return rel_bwd<m()>(tb, gr, sample, B, dS, ld, scale, P, ws, st); });
}

}  // namespace mkb

using namespace mkb;

extern "C" int64_t mkb_rel_step_workspace_bytes(const mkb_tables_t *tb, int64_t B) {
    RelPlan P;
    int rc;
    if (!tb || B <= 0 || !rel_plan(tb, B, P, &rc)) return 0;
    return (int64_t)P.total;
}

extern "C" int mkb_rel_score_bwd(const mkb_tables_t *tb, const mkb_grads_t *gr, const int64_t *sample, int64_t B, const float *dscore,
                                 int64_t ld, void *ws, int64_t ws_bytes, void *stream) {
    if (int rc = validate_tables(tb)) return rc;
    MKB_REQUIRE(gr && gr->g_ent && gr->g_rel && sample && dscore, "null pointer");
    MKB_REQUIRE(tb->model != MKB_PROTATE || gr->g_modulus, "pRotatE needs g_modulus");
    MKB_REQUIRE(B >= 0, "B must be >= 0");
    MKB_REQUIRE(ld >= tb->n_relation && (B == 0 || ld <= INT32_MAX / B), "need ld >= n_relation and B * ld below 2^31");
    if (int rc = slot_rows_check(tb)) return rc;
    if (B == 0) return MKB_OK;
    RelPlan P;
    if (int rc = rel_check(tb, B, ws, ws_bytes, P)) return rc;
    return rel_bwd_dispatch(tb, gr, sample, B, dscore, ld, 1.f, P, ws, (hipStream_t)stream);
}

extern "C" int mkb_rel_step(const mkb_tables_t *tb, const mkb_grads_t *gr, const int64_t *sample, const float *weight, int64_t B,
                            float temperature, float lambda, const float *weight_sum, float *loss, float *pos, void *ws, int64_t ws_bytes,
                            void *stream) {
    if (int rc = validate_tables(tb)) return rc;
    MKB_REQUIRE(gr && gr->g_ent && gr->g_rel && sample && loss && pos, "null pointer");
    MKB_REQUIRE(tb->model != MKB_PROTATE || gr->g_modulus, "pRotatE needs g_modulus");
    MKB_REQUIRE(B >= 0, "B must be >= 0");
    MKB_REQUIRE(temperature - temperature == 0.f && temperature > 0.f, "the softmax temperature must be finite and > 0");
    MKB_REQUIRE(lambda - lambda == 0.f && lambda > 0.f, "lambda must be finite and > 0");
    if (int rc = slot_rows_check(tb)) return rc;
    if (B == 0) return MKB_OK;
    RelPlan P;
    if (int rc = rel_check(tb, B, ws, ws_bytes, P)) return rc;
    hipStream_t st = (hipStream_t)stream;
    unsigned char *b = (unsigned char *)ws;
    float *S = (float *)b, *scratch = (float *)(b + P.scr_off);
    const int64_t R = tb->n_relation;
    if (int rc = launch_slot_scores(tb, sample, B, nullptr, 0, R, false, S, R, st)) return rc;
    all_softmax_launch(S, B, R, R, sample + 1, 3, weight, weight_sum, temperature, loss, pos, scratch, st);
    hipLaunchKernelGGL(rel_scale_kernel, dim3(1), dim3(64), 0, st, loss, lambda);
    return rel_bwd_dispatch(tb, gr, sample, B, S, R, lambda, P, ws, st);
}
