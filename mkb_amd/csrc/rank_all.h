// The all-entity score block S = score(q_i, every entity) of B queries, written once: the evaluation (rank.hip: filtered ranks and
// top k) and the 1vsAll training step (score_all.hip: the softmax over the whole row and its backward) both call run_rank and hand
// it the launches that read S.  Three routes, chosen here and nowhere else:
//   RotatE / TransE:     the pooled forward's outer-product register tile, the "pool" being every entity in order;
//   ComplEx / DistMult:  ONE matrix-core product Q . E^T planned by plan_gemm (gemm_plan.h) with this route's limits -- no partial
//                        buffer, no K split -- and the three MKB_GEMM_* switches, read once per call;
//   anything else:       all_fwd_kernel, the lane-owns-dims tiling of the pooled forward (8 rows per 1024-lane workgroup, swap/DPP
//                        wave reduction, LDS cross-wave combine per 16 candidates) over consecutive table rows, split into slices
//                        over grid.y.
#pragma once
#include "common.h"
#include "query_side.h"
#include "score_pool_tile.h"  // the pooled forward's outer-product register tile, for the all-entity block of RotatE / TransE
#include "gemm_mfma.h"        // ... and the matrix-core product for ComplEx / DistMult, whose score is a dot product
#include "all_plan.h"         // ... its shape and limits

namespace mkb {

constexpr int kWGr = 1024, kWavesR = 16, TIr = 8, kSlabR = 16;

struct AllArgs {
    const float *ent, *Q;
    float *S;  // [B, N]
    const float *modulus;
    int B, d;
    int64_t N, De;
    float kd, c0, c1;
};

// NW waves per workgroup: 16 x KPT units per lane cover rows of up to 1024 KPT units; rows of <= 1024 units take 8 waves x 2 units
// per lane instead of 16 x 1 (round 5: the per-candidate wave reduction -- ~30 cross-lane operations -- is then paid once per 128
// units instead of once per 64, and the complex modulus runs on the packed pair form: the all-entity block of the headline
// model 4.5 -> 3.7 ms, the filtered evaluation of FB15k-237's test split 0.22 -> 0.19 s)
template <int MODEL, bool HEAD, int KPT, int NW = kWavesR>
__global__ __launch_bounds__(NW * 64) void all_fwd_kernel(AllArgs A) {
    constexpr bool CP = ModelTraits<MODEL>::cplx_pair;
    __shared__ float s_part[2][kSlabR][NW][TIr];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i0 = blockIdx.x * TIr;
    const int NU = CP ? A.d : (int)A.De;
    const int u0 = tid * KPT;
    float q0[TIr][KPT], q1[TIr][KPT];
#pragma unroll
    for (int r = 0; r < TIr; ++r)
#pragma unroll
        for (int v = 0; v < KPT; ++v) {
            const bool ok = (i0 + r < A.B) && (u0 + v < NU);
            const float *qrow = A.Q + (int64_t)min(i0 + r, A.B - 1) * A.De;
            const int uu = min(u0 + v, NU - 1);
            const float l0 = qrow[uu], l1 = CP ? qrow[A.d + uu] : 0.f;
            q0[r][v] = ok ? l0 : 0.f;
            q1[r][v] = ok ? l1 : 0.f;
        }
    const int64_t per = (A.N + gridDim.y - 1) / gridDim.y;
    const int64_t e_lo = (int64_t)blockIdx.y * per;
    const int64_t e_hi = min(A.N, e_lo + per);
    const int n_mine = (int)max((int64_t)0, e_hi - e_lo);
    for (int j = 0; j < n_mine; ++j) {
        const float *x = A.ent + (e_lo + j) * A.De;
        float x0[KPT], x1[KPT];
#pragma unroll
        for (int v = 0; v < KPT; ++v) {
            const bool ok = u0 + v < NU;
            const int uu = min(u0 + v, NU - 1);
            const float l0 = x[uu], l1 = CP ? x[A.d + uu] : 0.f;
            x0[v] = ok ? l0 : 0.f;
            x1[v] = ok ? l1 : 0.f;
        }
        float part[TIr];
#pragma unroll
        for (int r = 0; r < TIr; ++r) {
            part[r] = 0.f;
            if constexpr (CP && KPT % 2 == 0) {
                f2 acc = pair_term_cmod2(f2{q0[r][0], q0[r][1]}, f2{q1[r][0], q1[r][1]}, f2{x0[0], x0[1]}, f2{x1[0], x1[1]});
#pragma unroll
                for (int v = 2; v < KPT; v += 2)
                    acc += pair_term_cmod2(f2{q0[r][v], q0[r][v + 1]}, f2{q1[r][v], q1[r][v + 1]}, f2{x0[v], x0[v + 1]}, f2{x1[v], x1[v + 1]});
                part[r] = acc.x + acc.y;
            } else {
#pragma unroll
                for (int v = 0; v < KPT; ++v) {
                    if constexpr (CP) part[r] += pair_term_cmod(Cplx{q0[r][v], q1[r][v]}, Cplx{x0[v], x1[v]});
                    else part[r] += pair_term_real<MODEL, HEAD>(q0[r][v], x0[v], A.kd);
                }
            }
        }
        float t0, t1;
        reduce8_wave(part, t0, t1);
        const int jj = j % kSlabR, buf = (j / kSlabR) & 1;
        if ((lane & 15) == 0) {
            const int R = lane >> 4, r = 4 * (R >> 1) + 2 * (R & 1);
            s_part[buf][jj][wave][r] = t0;
            s_part[buf][jj][wave][r + 1] = t1;
        }
        if (jj == kSlabR - 1 || j == n_mine - 1) {
            __syncthreads();
            const int j0 = j - jj, nb = jj + 1;
            if (tid < nb * TIr) {
                const int cj = tid % nb, r = tid / nb;  // consecutive lanes -> consecutive candidates (coalesced store)
                if (i0 + r < A.B) {
                    float sum = 0.f;
#pragma unroll
                    for (int w = 0; w < NW; ++w) sum += s_part[buf][cj][w][r];
                    if constexpr (MODEL == MKB_PROTATE) sum *= A.modulus[0];
                    A.S[(int64_t)(i0 + r) * A.N + e_lo + j0 + cj] = A.c0 + A.c1 * sum;
                }
            }
        }
    }
}

// scores_out[i, e] = c0 + c1 * S[i * ld + e]: the finished score block the ranks were counted on, for callers that want the
// scores themselves (mkb_rank_scores, mkb_all_score_fwd)
static __global__ __launch_bounds__(256) void export_scores_kernel(const float *__restrict__ S, float *__restrict__ out, int64_t N,
                                                                   int64_t ld, float c0, float c1) {
    const int64_t i = blockIdx.y;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < N; e += (int64_t)gridDim.x * 256) out[i * N + e] = c0 + c1 * S[i * ld + e];
}

// ids[i] = min(i, n_real - 1) for i < n (n >= n_real: the padded tail repeats the last row)
static __global__ __launch_bounds__(256) void iota_kernel(int64_t *ids, int64_t n, int64_t n_real) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) ids[i] = i < n_real ? i : n_real - 1;
}

// The all-entity score block of B queries into S on one of three routes, then `finish(c0, c1, ld)`: the launch(es) that read S (the
// filtered ranks of mkb_rank / mkb_rank_scores, the filtered top k of mkb_topk, the row softmax of the 1vsAll step).  S holds raw
// pair sums (tile route) or finished scores, ld floats apart; the finisher applies c0 + c1 * S[e].  On the matrix-core route
// ld = Npad = N rounded up to a multiple of 4 and ids [Npad] is left holding 0 .. N - 1 followed by N - 1 repeated: columns
// N .. Npad - 1 of S then hold the last entity's score again.
template <int MODEL, bool HEAD, class Finish>
static int run_rank(const mkb_tables_t *tb, const int64_t *sample, int64_t B, float *Q, float *S, int64_t *ids, hipStream_t st,
                    const Finish &finish) {
    const RowArgs ra = query_build_args(tb->ent, tb->rel, sample, Q, tb->entity_dim, tb->relation_dim, tb->hidden_dim, B, tb->phase_div);
    hipLaunchKernelGGL((query_build_kernel<MODEL, HEAD>), dim3((unsigned)B), dim3(256), 0, st, ra);
    const float c0 = ModelTraits<MODEL>::uses_gamma ? tb->gamma : 0.f, c1 = ModelTraits<MODEL>::uses_gamma ? -1.f : 1.f;
    // RotatE / TransE: the all-entity block on the pooled forward's register tile (score_pool_tile.h: 64 queries x 64 entities per
    // workgroup, 4 x 4 pairs per lane, operands staged through LDS -- no per-candidate wave reduction at all), the "pool" being
    // every entity in order and nothing masked; S then holds raw pair sums, finished by the rank kernel.
    if constexpr (ModelTraits<MODEL>::cplx_pair || MODEL == MKB_TRANSE) {
        const bool shape_ok = ModelTraits<MODEL>::cplx_pair ? (tb->hidden_dim % 4 == 0 && tb->hidden_dim >= 32)
                                                            : (tb->entity_dim % 4 == 0 && tb->entity_dim >= 64);
        if (shape_ok && (((uintptr_t)tb->ent | (uintptr_t)Q | (uintptr_t)S) & 15) == 0 && ids && tb->n_entity < (1 << 30)) {
            hipLaunchKernelGGL(iota_kernel, dim3((unsigned)((tb->n_entity + 255) / 256)), dim3(256), 0, st, ids, tb->n_entity, tb->n_entity);
            PoolArgs P{};
            P.ent = tb->ent; P.Q = Q; P.pool = ids; P.B = (int)B; P.P = (int)tb->n_entity; P.d = tb->hidden_dim; P.De = tb->entity_dim;
            P.kd = tb->phase_div; P.c0 = c0; P.c1 = c1;
            TileArgs T{};
            T.part = S; T.Kd = (int)tb->n_entity; T.ks = 1;
            T.row_tiles = (int)((B + kTileRows - 1) / kTileRows); T.pos_tiles = (int)((tb->n_entity + kTilePos - 1) / kTilePos);
            hipLaunchKernelGGL((pool_fwd_tile_kernel<MODEL, HEAD, 2>), dim3((unsigned)(T.row_tiles * T.pos_tiles)), dim3(256), 0, st, P, T);
            finish(c0, c1, tb->n_entity);
            MKB_LAUNCH_CHECK();
            return MKB_OK;
        }
    }
    // ComplEx / DistMult: score = <q, x> over the entity row, so the all-entity block is ONE product Q [B, De] . E^T [De, N] on the
    // matrix cores (gemm_mfma.h: 128-row tiles, fp32 operands split three ways on the bf16 pipe as in the pooled forward of these
    // models).  N is padded to a multiple of 4 through the id list (the tail repeats the last row; the rank kernel never reads it),
    // S rows are Npad floats apart.  Ragged last batches (B % 4 != 0) keep the lane-owns-dims kernel.
    if constexpr (MODEL == MKB_COMPLEX || MODEL == MKB_DISTMULT) {
        const int64_t Npad = all_npad(tb->n_entity);
        if (all_fwd_on_gemm(B, tb->n_entity, tb->entity_dim, (((uintptr_t)tb->ent | (uintptr_t)Q | (uintptr_t)S) & 15) == 0, ids != nullptr)) {
            hipLaunchKernelGGL(iota_kernel, dim3((unsigned)((Npad + 255) / 256)), dim3(256), 0, st, ids, Npad, tb->n_entity);
            // (shape and limits: all_plan.h -- one [B, Npad] block, no partial buffer, no K split)
            const GemmPlan plan = plan_gemm(all_fwd_shape(B, tb->n_entity, tb->entity_dim), all_fwd_limits(), gemm_switches_from_env());
            GemmArgs G = gemm_args(plan);
            G.A = Q; G.B = tb->ent; G.C = S; G.b_idx = ids; G.c0 = c0; G.c1 = c1;
            if (int rc = launch_gemm<true, true, GEMM_STORE_AFFINE>(plan, G, st)) return rc;
            finish(0.f, 1.f, Npad);
            MKB_LAUNCH_CHECK();
            return MKB_OK;
        }
    }
    AllArgs A{tb->ent, Q, S, tb->modulus, (int)B, tb->hidden_dim, tb->n_entity, tb->entity_dim, tb->phase_div, c0, c1};
    const int tiles = (int)((B + TIr - 1) / TIr);
    int slices = (512 + tiles - 1) / tiles;  // aim for >= 2 workgroups per CU
    if (slices < 1) slices = 1;
    if ((int64_t)slices > tb->n_entity) slices = (int)tb->n_entity;
    dim3 grid((unsigned)tiles, (unsigned)slices);
    const int NU = tb->model == MKB_ROTATE ? tb->hidden_dim : (int)tb->entity_dim;
    if (NU <= kWGr / 2) hipLaunchKernelGGL((all_fwd_kernel<MODEL, HEAD, 1>), grid, dim3(kWGr), 0, st, A);
    else if (NU <= kWGr) hipLaunchKernelGGL((all_fwd_kernel<MODEL, HEAD, 2, 8>), grid, dim3(512), 0, st, A);
    else if (NU <= 2 * kWGr) hipLaunchKernelGGL((all_fwd_kernel<MODEL, HEAD, 2>), grid, dim3(kWGr), 0, st, A);
    else hipLaunchKernelGGL((all_fwd_kernel<MODEL, HEAD, 4>), grid, dim3(kWGr), 0, st, A);
    finish(0.f, 1.f, tb->n_entity);
    MKB_LAUNCH_CHECK();
    return MKB_OK;
}

}  // namespace mkb
