// The three matrix-core products of the all-entity block of ComplEx / DistMult as plan_gemm sees them: shapes and limits, written
// once.  The forward S = Q . E^T is the evaluation's (run_rank, rank_all.h); the 1vsAll step (score_all.hip) adds the two backward
// products.  Plain host code, like gemm_plan.h: a host program can ask the planner which kernel family a table shape gets.
#pragma once
#include "gemm_plan.h"

namespace mkb {

// N rounded up to a multiple of 4: the forward pads the entity list by repeating the last entity
inline int64_t all_npad(int64_t N) { return (N + 3) & ~(int64_t)3; }

// ---- forward: S [B, Npad] = Q [B, De] . E[ids]^T.  Ragged batches (B % 4 != 0), short or unaligned rows and tables without an id
// list keep the lane-owns-dims kernel.
inline bool all_fwd_on_gemm(int64_t B, int64_t N, int64_t De, bool aligned16, bool have_ids) {
    return have_ids && B % 4 == 0 && De % 4 == 0 && De >= 16 && B >= 32 && aligned16 && all_npad(N) < (1 << 30);
}
inline GemmShape all_fwd_shape(int64_t B, int64_t N, int64_t De) {
    const int64_t Npad = all_npad(N);
    return GemmShape{(int)B, (int)Npad, (int)De, De, De, Npad, true, true, GEMM_STORE_AFFINE, true, N};
}
// The workspace holds ONE [B, Npad] score block and no partial buffer: max_ks = 1 -- a K split would write its partial products
// past S (over the id list this very product gathers through).
inline GemmLimits all_fwd_limits() { return GemmLimits{false, 0, 0, /*max_ks=*/1, false}; }

// ---- dQ [B, De] = dS [B, ld] . E: the pooled dQ with every entity as the pool.  gathered: dS is the forward's padded block
// (ld = Npad > N, pad columns exactly 0) and K runs over the forward's id list, which keeps K a multiple of 4; otherwise K = N over
// the table itself.
inline GemmShape all_dq_shape(int64_t B, int64_t N, int64_t De, int64_t ld, bool gathered, bool aligned16) {
    return GemmShape{(int)B, (int)De, (int)(gathered ? all_npad(N) : N), ld, De, De, true, false, GEMM_STORE, aligned16, N};
}
constexpr int kAllMaxKs = 4;
inline GemmLimits all_dq_limits() { return GemmLimits{true, 0, 0, kAllMaxKs, false}; }

// ---- dE [N, De] += dS^T . Q: M = N (not Npad: every row of C is a row of the gradient table), K = B.  A table that fills the chip
// with 64-row tiles is never split (the planner's own rule): then no partial buffer is kept for it -- max_ks copies of the entity
// table -- and only small tables get one.
inline GemmShape all_de_shape(int64_t B, int64_t N, int64_t De, int64_t ld, bool aligned16) {
    return GemmShape{(int)N, (int)De, (int)B, ld, De, De, false, false, GEMM_ACCUM, aligned16, B};
}
inline GemmLimits all_de_limits(int64_t N, int64_t De) {
    const bool fills = ((N + 63) / 64) * ((De + 63) / 64) >= 768;
    return fills ? GemmLimits{false, 0, 0, 1, false} : GemmLimits{true, 0, 0, kAllMaxKs, false};
}

}  // namespace mkb
