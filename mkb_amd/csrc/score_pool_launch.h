// Launch helpers of the pooled tile kernels: PoolPlan + PoolArgs -> grid, block, LDS.  Included by score_pool_<model>.hip,
// which instantiate pool_launch for their model.
#pragma once
#include "score_pool_plan.h"
#include "score_pool_tile.h"

namespace mkb {

// the row-tile forward (fwd) or the two-pass backward for one (units per lane, waves) workgroup shape
template <int MODEL, bool HEAD, int KPT, int NW>
static int launch_cfg(bool fwd, const PoolPlan &L, const PoolArgs &A, hipStream_t st) {
    const dim3 block(NW * 64);
    if (fwd) {
        const dim3 grid((unsigned)((A.B + TI - 1) / TI), (unsigned)L.rows.slices);
        hipLaunchKernelGGL((pool_fwd_kernel<MODEL, HEAD, KPT, NW>), grid, block, (size_t)3 * ((A.P + L.rows.slices - 1) / L.rows.slices) * 4, st, A);
    } else if constexpr (pool_two_pass_compiled(MODEL, KPT)) {
        const size_t rows_per = (size_t)((A.B + L.two.x_slices - 1) / L.two.x_slices);
        const size_t lds_x = ((TI + 2) * rows_per + 16) * 4;
        const size_t lds_q = ((size_t)(TI + 2) * ((A.P + L.two.q_slices - 1) / L.two.q_slices) + 32) * 4;
        const unsigned xb = (unsigned)(((A.P + TI - 1) / TI) * L.two.x_slices);
        const unsigned qb = (unsigned)(((A.B + TI - 1) / TI) * L.two.q_slices);
        PoolArgs A2 = A;  // (the two fields that depend on this launch's grid)
        A2.x_blocks = (int)xb;
        // dq workgroups ahead of the dx pass: a little under one per CU measured best (headline: 0 -> 169 us, 96..224 ->
        // 160-165 us, 256 -> 170 us; the other shapes are flat within 2 %)
        A2.q_first = (int)(qb < 160u ? qb : 160u);
        hipLaunchKernelGGL((pool_bwd_kernel<MODEL, HEAD, KPT, NW>), dim3(xb + qb), block, lds_x > lds_q ? lds_x : lds_q, st, A2);
    } else {
        return set_error(MKB_ERR_UNSUPPORTED, "two-pass pooled backward not compiled for this model at %d units per lane", KPT);
    }
    MKB_LAUNCH_CHECK();
    return MKB_OK;
}

template <int MODEL, bool HEAD, int KPT>
static int launch_bwd1(const Bwd1Layout &Y, const PoolArgs &A, hipStream_t st) {
    // the dense form is compiled for the complex-modulus pair function and for TransE (the plan never asks for it elsewhere:
    // DistMult / ComplEx take the matrix route, pRotatE's term is two transcendental chains; every instantiation is ~60 KB)
    constexpr bool kHasDense = ModelTraits<MODEL>::cplx_pair || MODEL == MKB_TRANSE;
    const bool dense = kHasDense && Y.dense_lanes > 0;
    if (!kHasDense && Y.dense_lanes > 0) return set_error(MKB_ERR_INVALID, "the dense pass is built for the complex-modulus models and TransE only");
    const size_t lds = Y.lds_bytes();
    static LdsOptIn lds_ok[2];  // per instantiation: opt in to more than 64 KB of dynamic LDS once per device
    if (lds > 64 * 1024) {
        const void *fn = reinterpret_cast<const void *>(&pool_bwd1_kernel<MODEL, HEAD, KPT, false>);
        if constexpr (kHasDense)
            if (dense) fn = reinterpret_cast<const void *>(&pool_bwd1_kernel<MODEL, HEAD, KPT, true>);
        if (int rc = lds_ok[dense].ensure(fn, 160 * 1024)) return rc;
    }
    bool launched = false;
    if constexpr (kHasDense)
        if (dense) {
            hipLaunchKernelGGL((pool_bwd1_kernel<MODEL, HEAD, KPT, true>), dim3(Y.grid()), dim3(kBwd1Waves * 64), lds, st, A);
            launched = true;
        }
    if (!launched)
        hipLaunchKernelGGL((pool_bwd1_kernel<MODEL, HEAD, KPT, false>), dim3(Y.grid()), dim3(kBwd1Waves * 64), lds, st, A);
    const DxReduce R = Y.dx_reduce(A);
    if (A.dx_reduce_out) *A.dx_reduce_out = R;  // the caller's next launch (row backward) carries the reduction
    else hipLaunchKernelGGL(pool_dx_reduce_kernel<0>, dim3((unsigned)R.blocks), dim3(256), 0, st, R);
    MKB_LAUNCH_CHECK();
    return MKB_OK;
}

template <int MODEL, bool HEAD, int KPT>
static int launch_wave(const PoolPlan &L, const PoolArgs &A, hipStream_t st) {
    const dim3 grid((unsigned)((A.B + TI - 1) / TI), (unsigned)L.wave.slices, (unsigned)L.wave.chunks);
    hipLaunchKernelGGL((pool_bwd_wave_kernel<MODEL, HEAD, KPT>), grid, dim3(64), 0, st, A);
    MKB_LAUNCH_CHECK();
    return MKB_OK;
}

template <int MODEL, bool HEAD>
int pool_launch(int which, const PoolPlan &L, const PoolArgs &A, hipStream_t st) {
    const bool fwd = which == kPoolFwd;
    if (fwd && L.fwd == FwdRoute::Tile) return launch_fwd_tile<MODEL, HEAD>(L, A, st, A.tile_part, A.tile_tail);
    if (!fwd && L.bwd == BwdRoute::Wave) return L.wave.kpt == 2 ? launch_wave<MODEL, HEAD, 2>(L, A, st) : launch_wave<MODEL, HEAD, 1>(L, A, st);
    if (!fwd && L.bwd == BwdRoute::SinglePass) {
        if constexpr (!ModelTraits<MODEL>::cplx_pair && MODEL != MKB_PROTATE)
            if (L.single.kpt == 4) return launch_bwd1<MODEL, HEAD, 4>(L.single, A, st);
        return L.single.kpt >= 2 ? launch_bwd1<MODEL, HEAD, 2>(L.single, A, st) : launch_bwd1<MODEL, HEAD, 1>(L.single, A, st);
    }
    if (fwd ? L.fwd != FwdRoute::RowTile : L.bwd != BwdRoute::TwoPass) return set_error(MKB_ERR_INVALID, "no pooled tile kernel for this plan (kernel %d)", which);
    // the (units per lane, waves) workgroup shapes the row-tile forward and the two-pass backward are compiled for
    const int kpt = fwd ? L.rows.kpt : L.kpt, nw = fwd ? L.rows.nw : L.nw;
    if (kpt == 1 && nw == 1) return launch_cfg<MODEL, HEAD, 1, 1>(fwd, L, A, st);
    if (kpt == 2 && nw == 1) return launch_cfg<MODEL, HEAD, 2, 1>(fwd, L, A, st);
    if (kpt == 1 && nw == 2) return launch_cfg<MODEL, HEAD, 1, 2>(fwd, L, A, st);
    if (kpt == 1 && nw == 4) return launch_cfg<MODEL, HEAD, 1, 4>(fwd, L, A, st);
    if (kpt == 1 && nw == 16) return launch_cfg<MODEL, HEAD, 1, 16>(fwd, L, A, st);
    if (kpt == 2 && nw == 2) return launch_cfg<MODEL, HEAD, 2, 2>(fwd, L, A, st);
    if (kpt == 2 && nw == 4) return launch_cfg<MODEL, HEAD, 2, 4>(fwd, L, A, st);
    if (kpt == 2 && nw == 8) return launch_cfg<MODEL, HEAD, 2, 8>(fwd, L, A, st);
    if (kpt == 2 && nw == 16) return launch_cfg<MODEL, HEAD, 2, 16>(fwd, L, A, st);
    // (pRotatE's pair term carries a sin / cos and two divisions: its 4-units-per-lane bodies are 230 KB of code each and
    // were a seventh of the library; the plan keeps that model at <= 2 units per lane)
    if constexpr (MODEL != MKB_PROTATE) {
        if (kpt == 4 && nw == 4) return launch_cfg<MODEL, HEAD, 4, 4>(fwd, L, A, st);
        if (kpt == 4 && nw == 16) return launch_cfg<MODEL, HEAD, 4, 16>(fwd, L, A, st);
    }
    return set_error(MKB_ERR_UNSUPPORTED, "no pooled kernel configuration (kpt=%d, nw=%d)", kpt, nw);
}

}  // namespace mkb
