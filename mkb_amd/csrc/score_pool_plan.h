// Launch plan of the pooled scoring path: which kernel runs for a table shape, with which grid, over which workspace
// layout.  plan_pool (below) fills a PoolPlan, score_pool.hip carves the workspace from it; score_pool_launch.h launches the VALU
// routes from it, gemm_mfma.h the matrix route's three products (their GemmPlans, gemm_plan.h, are part of the plan).
#pragma once
#include <algorithm>
#include "gemm_plan.h"
#include "score_pool_kernels.h"

namespace mkb {

// The per-call switches (DESIGN.md "Run-time switches").  They change the routes and with them the workspace layout, so an
// ABI entry point reads them once and every decision of that call is taken from the one value.
struct PoolSwitches {
    enum Dense { kDenseDefault, kDenseOff, kDenseOn };
    bool no_mfma;  // MKB_POOL_NO_MFMA=1: the bilinear models keep the VALU kernels (the tests' independent route)
    Dense dense;   // MKB_POOL_DENSE: the dense pass of the single-pass backward (default: on where the model has the form)
    GemmSwitches gemm;  // MKB_GEMM_NO128 / MKB_GEMM_NO_PAIR / MKB_GEMM_BF16X3: the matrix route's products (gemm_plan.h)
};

// Which tails of the matrix route's products the call folds into its next launch: the split-K sum of the scores into the loss
// rows (mkb_pool_step), the scattered add of dX into the row backward (mkb_pool_step and mkb_pool_step_bwd).  A folding product
// asks for twice the workgroups, so its K split -- not the workspace layout -- depends on these.
struct PoolFolds { bool s, x; };

enum class FwdRoute {
    Matrix,   // S = Q . ent[pool]^T on the matrix cores (gemm_mfma.h; ComplEx / DistMult)
    Tile,     // dense prefix on the outer-product register tile + sparse fringe (pool_fwd_tile_kernel)
    RowTile,  // row tiles of 8 x position slices (pool_fwd_kernel)
};
enum class BwdRoute {
    Matrix,      // two products on the matrix cores (gemm_mfma.h)
    SinglePass,  // every pair term evaluated once (pool_bwd1_kernel) + the dx partial reduction
    Wave,        // a small problem: one wave per piece (pool_bwd_wave_kernel)
    TwoPass,     // dq and dx passes in one grid (pool_bwd_kernel): pools of more positions than the single-pass kernel has blocks for
};

// The two-pass backward takes 4 floats per lane and position: RotatE at >= 2 units per lane, or a real-valued model at 4
// (pRotatE has no 4-unit form).  It is compiled for these (model, units per lane) pairs alone.
constexpr bool pool_two_pass_compiled(int model, int kpt) { return model != MKB_PROTATE && kpt >= 2; }

// Blocked layout of the single-pass backward.  Dims are cut into slices of 64 * kpt units, positions into `blocks` blocks of
// halves * 64 slots (position p = block + blocks * (lane * halves + half)), row tiles of 8 into groups of 16 waves x
// tiles_per_wave.  The seeds G, the dx partials, the used-slot masks, the kernel's LDS and its grid all follow from these.
struct Bwd1Layout {
    int blocks, halves;  // powers of two: the kernel cuts its 16 chunks into 16 / halves lanes per half, the seed layout shifts by their log2
    int dim_slices, kpt, cplx;
    int tiles_per_wave, row_groups;
    int dense_lanes;     // lanes [0, dense_lanes) of every half hold positions of the dense prefix (0 = the general pass)

    int nc() const { return kpt * (cplx ? 2 : 1); }  // floats per lane and position
    // halves the LDS accumulator (<= 128 KB) holds: 2 at nc = 4, 4 at nc = 2, 8 at nc = 1
    static int max_halves(int nc) { return 128 * 1024 / (64 * nc * 64 * 4); }
    // halves of 64 slots that cover the P positions of `blocks` blocks, ROUNDED UP to a power of two: 3, 5, 6, 7 would break
    // the kernel's chunk split and the seed layout's shifts (e.g. TransE hidden 500, B 2048, K 384: 192 positions per block
    // = 3 halves).  max_halves is a power of two, so the rounded value still fits; slots past P are masked in the kernel.
    static int halves_for(int64_t P, int blocks) {
        const int need = (int)(((P + blocks - 1) / blocks + 63) / 64);
        int h = 1;
        while (h < need) h *= 2;
        return h;
    }
    bool valid() const {
        return blocks > 0 && (blocks & (blocks - 1)) == 0 && halves > 0 && (halves & (halves - 1)) == 0 && halves <= max_halves(nc());
    }

    int slots() const { return blocks * halves * 64; }
    SeedLayout seeds() const { return SeedLayout{__builtin_ctz((unsigned)blocks), __builtin_ctz((unsigned)halves)}; }
    // rows are padded to tiles of 8: the dense pass reads a tile's 8 seeds without looking at B
    static int64_t padded_rows(int64_t B) { return (B + 7) / 8 * 8; }
    size_t seed_elems(int64_t B) const { return (size_t)padded_rows(B) * slots(); }
    // dx partials [row groups][blocks][slots][dim slices][64 lanes][nc] and used-slot masks [row groups][blocks][8]
    size_t dxp_elems() const { return (size_t)row_groups * slots() * dim_slices * 64 * nc(); }
    size_t xused_words() const { return (size_t)row_groups * blocks * 8; }
    // dense pass: accumulator + row images of the dense slots, then reused for the workgroup's query rows
    size_t lds_main() const {
        const size_t pass = (size_t)2 * halves * dense_lanes * nc() * 64 * 4;
        const size_t rows = tiles_per_wave == 1 ? (size_t)kBwd1Waves * TI * nc() * 64 * 4 : 0;
        return pass > rows ? pass : rows;
    }
    int lds_ids_off() const { return (int)(lds_main() / 4); }  // the block's pool-id table sits behind them
    size_t lds_bytes() const {
        return dense_lanes > 0 ? lds_main() + 128 + (size_t)halves * 64 * 8 : (size_t)halves * 64 * nc() * 64 * 4 + 128;
    }
    unsigned grid() const { return (unsigned)row_groups * blocks * dim_slices; }
    DxReduce dx_reduce(const PoolArgs &A) const {
        DxReduce R{};
        R.dXp = A.dXp; R.xused = A.xused; R.pool = A.pool; R.g_ent = A.g_ent; R.De = A.De; R.P = A.P; R.d = A.d;
        R.npb = blocks; R.halves = halves; R.dim_slices = dim_slices; R.row_groups = row_groups; R.kpt = kpt;
        R.cplx = cplx; R.blocks = slots();
        return R;
    }
};

// Route parameters: a plan holds only those of its routes
struct FwdRows { int kpt, nw, slices; };             // units per lane (it amortises its wave reduction over more of them), waves, position slices
struct FwdTile { int kpt, kd, ks, fringe_slices; };  // dense prefix [0, kd) in ks dim splits, the fringe's position slices (score_pool_tile.h)
struct BwdWave { int kpt, chunks, slices; };         // units per lane, dim chunks, position slices
struct BwdTwoPass { int q_slices, x_slices; };       // dQ slices of the dq pass, row slices of the dx pass
struct BwdMatrix { GemmPlan dq, dx; bool pair; };    // dQ = G . ent[pool] into <= kMfmaDqSlices slices, dX = G^T . Q scattered; pair: ONE launch

struct PoolPlan {
    // row kernels
    int rel_copies;     // > 1: copies of the relation gradient the row backward spreads its atomics over (few relations)
    int64_t rel_elems;  // n_relation * relation_dim
    int64_t n_entity;
    int kpt, nw;        // units per lane and waves per workgroup that cover a row

    FwdRoute fwd;
    union {
        GemmPlan gemm;  // Matrix
        FwdRows rows;   // RowTile
        FwdTile tile;   // Tile
    };

    BwdRoute bwd;
    int dq_parts;  // [B, De] partial buffers of dQ the row / query backward sums (Matrix: the slices of the dQ plan)
    // Matrix: floats of split-K partials the workspace holds -- the most any product of the route writes, whatever the call folds
    size_t gemm_part;
    union {
        BwdMatrix products;  // Matrix
        Bwd1Layout single;  // SinglePass (dq_parts = its position blocks)
        BwdWave wave;       // Wave (dq_parts = its position slices)
        BwdTwoPass two;     // TwoPass (dq_parts = its dQ slices)
    };

    bool matrix() const { return bwd == BwdRoute::Matrix; }
    bool single_pass() const { return bwd == BwdRoute::SinglePass; }
    SeedLayout seeds() const { return single_pass() ? single.seeds() : SeedLayout{-1, 0}; }
};

// The kernels pool_launch launches (its `which` argument)
constexpr int kPoolFwd = 0;  // forward, by the plan's forward route
constexpr int kPoolBwd = 1;  // backward, by the plan's backward route

// Defined in score_pool_launch.h and instantiated per model in score_pool_<model>.hip (the five families compile in parallel)
template <int MODEL, bool HEAD>
int pool_launch(int which, const PoolPlan &L, const PoolArgs &A, hipStream_t st);

// ------------------------------------------------------------------------------------------------ planning
// Plain host code: no launches, no environment.  tests/test_host_pool_routes.py builds a host program on these very functions.
static int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// What the plan's decisions know about a table row
struct RowShape {
    int NU;           // units per row: complex numbers for RotatE, floats otherwise
    bool cp, al16;    // RotatE's complex units; 16-byte aligned table
    bool k4;          // 4 units per lane possible (pRotatE: no 4-units-per-lane instantiations, see launch_shape)
    int row_tiles, pos_tiles;
};

// relation-gradient copies of the row backward: when a relation averages >= 16 rows of the batch, spread them so that
// ~4 rows share a copy, within 1 MB of scratch (WN18RR B = 1024: 11 relations -> 23 copies; FB15k-237: none)
static int plan_rel_copies(const mkb_tables_t *tb, int64_t B) {
    const int64_t rel_elems = tb->n_relation * tb->relation_dim;
    const int64_t per_rel = tb->n_relation > 0 ? B / tb->n_relation : 0;
    if (per_rel < 16 || rel_elems <= 0) return 1;
    int64_t c = per_rel / 4;
    const int64_t cap = (1 << 18) / rel_elems;  // 1 MB of floats
    if (c > cap) c = cap;
    if (c > 64) c = 64;
    return c >= 2 ? (int)c : 1;
}

// units per lane: vector loads + packed math need even dims; waves: smallest workgroup that covers the row
static bool plan_row_shape(const mkb_tables_t *tb, int64_t B, int64_t P, RowShape &R, PoolPlan &L) {
    const int64_t De = tb->entity_dim, d = tb->hidden_dim;
    R.NU = tb->model == MKB_ROTATE ? tb->hidden_dim : (int)tb->entity_dim;
    R.cp = tb->model == MKB_ROTATE;
    R.al16 = (((uintptr_t)tb->ent) & 15) == 0;
    const bool even2 = R.al16 && R.NU % 2 == 0 && De % 2 == 0 && (!R.cp || d % 2 == 0);
    const bool even4 = R.al16 && R.NU % 4 == 0 && De % 4 == 0 && (!R.cp || d % 4 == 0);
    R.k4 = even4 && tb->model != MKB_PROTATE;
    R.row_tiles = (int)((B + TI - 1) / TI);
    R.pos_tiles = (int)((P + TI - 1) / TI);
    if (even2 && R.NU >= 64 && R.NU <= 2048) L.kpt = 2;
    else if (R.k4 && R.NU > 2048 && R.NU <= 4096) L.kpt = 4;
    else if (R.NU <= 1024) L.kpt = 1;
    else return false;
    const int lanes = (R.NU + L.kpt - 1) / L.kpt;
    if (L.kpt == 1) L.nw = lanes <= 64 ? 1 : (lanes <= 128 ? 2 : (lanes <= 256 ? 4 : 16));
    else if (L.kpt == 2) L.nw = lanes <= 64 ? 1 : (lanes <= 128 ? 2 : (lanes <= 256 ? 4 : (lanes <= 512 ? 8 : 16)));
    else L.nw = 16;
    return true;
}

// ComplEx / DistMult: the pair function is a dot product, so the pooled block is three dense fp32 GEMMs on the matrix
// cores (gemm_mfma.h) instead of the lane-owns-dims VALU kernels.
static bool wants_matrix(const mkb_tables_t *tb, const PoolSwitches &sw) {
    return !sw.no_mfma && (tb->model == MKB_COMPLEX || tb->model == MKB_DISTMULT) && tb->entity_dim >= 16;
}

// The three products of the matrix route: S [B, P] = Q . ent[pool]^T, dQ [B, De] = G [B, P] . ent[pool] and the scattered
// dX [P, De] = G^T . Q.  Q, G and the partial buffer are workspace segments (256-byte aligned); the table is the caller's.
static void plan_matrix(const mkb_tables_t *tb, int64_t B, int64_t P, const RowShape &R, const PoolSwitches &sw, PoolFolds folds,
                        PoolPlan &L) {
    const int64_t De = tb->entity_dim;
    const GemmShape s_shape{(int)B, (int)P, (int)De, De, De, P, true, true, GEMM_STORE_AFFINE, R.al16, tb->n_entity};
    const GemmShape q_shape{(int)B, (int)De, (int)P, P, De, De, true, false, GEMM_STORE, R.al16, tb->n_entity};
    const GemmShape x_shape{(int)P, (int)De, (int)B, P, De, De, false, false, GEMM_ATOMIC_ROWS, true, B};
    // (a product whose tail rides the next launch asks for 2 workgroups per CU, want_wg = 500: the tail costs no launch)
    L.fwd = FwdRoute::Matrix;
    L.gemm = plan_gemm(s_shape, GemmLimits{true, 0, folds.s ? 500 : 0, 8, folds.s}, sw.gemm);
    L.bwd = BwdRoute::Matrix;
    // Both backward products in ONE launch where both take the 128-row bf16x3 tiles.  (Short rows -- DistMult's 1000 floats --
    // leave few tiles: split K further there: 26.5 -> 23.4 us for its pair; the 2000-float rows of ComplEx lose with more
    // splits, 42 -> 49 us: their partials are what the extra workgroups move.)
    const int pair_wg = De <= 1024 ? 400 : 200;
    BwdMatrix M{plan_gemm(q_shape, GemmLimits{true, kMfmaDqSlices, pair_wg, 8, false}, sw.gemm),
                plan_gemm(x_shape, GemmLimits{true, 0, pair_wg, 8, folds.x}, sw.gemm), true};
    M.pair = !sw.gemm.no_pair && M.dq.kernel == GemmKernel::Bf16x3Tile128 && M.dx.kernel == GemmKernel::Bf16x3Tile128;
    if (!M.pair) {
        // a K split of dQ leaves its partials in the dQ slices: the row backward sums them (it does so for the VALU route's
        // position blocks anyway) instead of a reduction launch in between (DistMult: 6.5 us)
        M.dq = plan_gemm(q_shape, GemmLimits{true, kMfmaDqSlices, 0, 8, false}, sw.gemm);
        M.dx = plan_gemm(x_shape, GemmLimits{true, 0, folds.x ? 500 : 0, 8, folds.x}, sw.gemm);
    }
    L.products = M;
    L.dq_parts = M.dq.slices();
    // room for the partials of whichever product runs, under every switch setting and whatever the call folds: callers cache
    // a workspace per table shape (mkb_pool_step_workspace_bytes), and the two halves of a step must carve the same layout.
    // (dQ is given the buffer too and counts with its bound, though with slices its K split lands in the dQ buffer: for
    // B >= P the room is then what it always was, 8 * B * max(P, De) floats; for B < P it grows to dX's 8 * P * De.)
    L.gemm_part = std::max({L.gemm.part_bound, M.dq.part_bound, M.dx.part_bound});
}

static void plan_forward(const mkb_tables_t *tb, int64_t B, int64_t P, const RowShape &R, const PoolSwitches &sw, PoolPlan &L) {
    // 4 units per lane when the row allows it (measured 91 -> 77 us at the headline shape: the per-position wave
    // reduction is amortised over twice the pair evaluations); the backward kernels gain nothing from it
    const bool wide = R.k4 && R.NU > 512 && R.NU <= 1024;
    const int fkpt = wide ? 4 : L.kpt, fnw = wide ? 4 : L.nw;
    // Complex-modulus models and TransE (its "dims" are pairs of floats, so that a chunk is 32 floats either way): dense
    // prefix [0, Kd) of the pool on the outer-product register tile, the sparse fringe on the row-tile kernel in the same
    // launch (score_pool_tile.h).  Needs the 4-wave forward configuration (rows of 257 .. 1024 complex dims), whole
    // 64-position tiles in the prefix (K = P / 2 >= 64) and 16-byte rows.
    const int64_t De = tb->entity_dim, d = tb->hidden_dim, Kd = (P / 2) / 64 * 64;
    const bool te = tb->model == MKB_TRANSE && De % 4 == 0;
    if ((te || (R.cp && d % 4 == 0)) && R.al16 && fnw == 4 && (fkpt == 4 || fkpt == 2) && Kd >= 64 && B >= 64) {
        const int64_t dt = R.cp ? d : De / 2;
        const int tiles = (int)((B + 63) / 64) * (int)(Kd / 64);
        int ks = 1;
        while (tiles * ks < 512 && ks < 16 && dt / (ks * 2) >= 32) ks *= 2;  // fill the chip; >= 2 chunks of 16 dims per split
        L.fwd = FwdRoute::Tile;
        L.tile = {fkpt, (int)Kd, ks, 2};
        return;
    }
    // ~32 waves per CU (short rows: 99 -> 79 us at the 8-GPU shard; flat at the headline shape)
    L.fwd = FwdRoute::RowTile;
    L.rows = {fkpt, fnw, clampi((256 * 32 / fnw + R.row_tiles - 1) / R.row_tiles, 1, kMaxSlices)};
}

// Slice counts of the two-pass backward, swept on the headline shape and on the dimension shards of 2 / 4 / 8 GPUs
// (tools/shard_emulate.py: rows grow, rows get shorter, workgroups shrink to 4 / 2 / 1 waves).
static void plan_two_pass(int64_t B, const RowShape &R, PoolPlan &L) {
    const int target = 256 * 16 / L.nw;  // workgroups for ~16 waves per CU
    // dq pass: it shares its launch with the dx pass, so with big workgroups half the waves suffice (headline: 2 slices
    // instead of 4 keep the merged kernel at 160 us and save row_bwd 4 us of partial-buffer reads); 1- and 2-wave
    // workgroups want the full count (8-GPU shard: 210 -> 185 us).
    const int q_target = L.nw >= 4 ? target / 2 : target;
    L.two.q_slices = clampi((q_target + R.row_tiles - 1) / R.row_tiles, 1, kMaxSlices);
    // x pass: rows of a slice are listed in LDS (40 B each): keep a slice <= 256 rows so several workgroups fit a CU;
    // single-wave workgroups do better with 256-row slices than with 128 (8-GPU shard: 209 -> 192 us)
    const int min_x = (int)((B + 255) / 256);
    const int x_target = L.nw == 1 ? target / 2 : target;
    L.two.x_slices = clampi((x_target + R.pos_tiles - 1) / R.pos_tiles, min_x > 2 ? min_x : 2, 1 << 20);
    L.dq_parts = L.two.q_slices;
}

// Small problems: when the single-pass grid would be a handful of 16-wave workgroups, its ring and its prologue ARE the
// launch (Umls TransE-64, K 16, B 256: two workgroups, 43 us for 0.5 MFLOP).  One wave per (row tile, <= 64 positions,
// 64 * kpt units) instead: pool_bwd_wave_kernel; position slices until ~1024 waves are in flight.
static bool plan_wave(int64_t P, const RowShape &R, const Bwd1Layout &Y, PoolPlan &L) {
    const int groups1 = (R.row_tiles + kBwd1Waves - 1) / kBwd1Waves;
    const int kpt = L.kpt >= 2 ? 2 : 1;
    const int chunks = (R.NU + 64 * kpt - 1) / (64 * kpt);
    int nsl = (int)((P + 63) / 64);
    while (nsl < kMaxSlices && (int64_t)R.row_tiles * chunks * nsl < 1024 && P / nsl > 2) ++nsl;
    if ((int64_t)groups1 * Y.blocks * Y.dim_slices > 32 || nsl > kMaxSlices) return false;
    L.wave = {kpt, chunks, nsl};
    L.dq_parts = nsl;
    return true;
}

// Dense pass (pool_bwd1_kernel<..., DENSE>).  Every row takes its first K = P / 2 surviving candidates, so positions
// p < K are used by (nearly) every row.  Slot (h, l) holds position block + blocks * (l * halves + h): lanes
// l < K / (blocks * halves) of every half are dense; rounded down to whole lanes per chunk (a chunk = every cph-th lane
// of a half).  DESIGN.md section 8: the same gradients; per step, same box, general vs dense pass:
// headline 0.242 -> 0.240 ms, WN18RR 0.150 -> 0.143, YAGO3-10 0.206 -> 0.202, TransE-1000 0.183 -> 0.185.  So: on
// for the complex-modulus pair function and for TransE (with its pair term down to 5 VALU operations the general pass's
// per-position bookkeeping is a quarter of the loop: 62.7 -> 59.5 us at the headline shape, same call); the other
// real-valued models have no dense form (their ten instantiations were 0.6 MB of the library for a path that measured slower).
static int plan_dense_lanes(const mkb_tables_t *tb, int64_t P, const Bwd1Layout &Y, const PoolSwitches &sw) {
    const bool dense_model = tb->model == MKB_ROTATE || tb->model == MKB_TRANSE;
    if (!dense_model || sw.dense == PoolSwitches::kDenseOff) return 0;
    const int cph = kChunks / Y.halves;
    const int ld = (int)((P / 2) / ((int64_t)Y.blocks * Y.halves)) / cph * cph;
    return cph >= 1 && ld > 0 && ld <= 32 ? ld : 0;
}

// VALU models.  Single-pass backward: position blocks are doubled until the halves fit the LDS accumulator, then until the
// grid holds ~4096 waves (16 per CU); each block costs one dQ partial buffer.  More blocks than dQ buffers: the two-pass
// kernel; a handful of workgroups: the wave kernel.
static bool plan_backward(const mkb_tables_t *tb, int64_t B, int64_t P, const RowShape &R, const PoolSwitches &sw, PoolPlan &L) {
    Bwd1Layout Y{};
    // units per lane: 2 (1 for odd rows); real-valued models with long rows take 4 -- the same 4 floats per lane and
    // position as RotatE's two complex dims, half the per-position bookkeeping of 2
    Y.kpt = (!R.cp && R.k4 && R.NU >= 512) ? 4 : (L.kpt >= 2 ? 2 : 1);
    Y.cplx = R.cp ? 1 : 0;
    Y.dim_slices = ((R.NU + Y.kpt - 1) / Y.kpt + 63) / 64;
    int npb = 1;
    while (Bwd1Layout::halves_for(P, npb) > Bwd1Layout::max_halves(Y.nc())) npb *= 2;
    while (npb < kMaxSlices && (int64_t)R.row_tiles * Y.dim_slices * npb < 4096 && (P + npb - 1) / npb > 32) npb *= 2;
    Y.blocks = npb;
    if (npb > kMaxSlices) {
        // (compiled only where a shape can reach it; the check keeps a route with no kernel from being picked)
        if (!pool_two_pass_compiled(tb->model, L.kpt)) return false;
        L.bwd = BwdRoute::TwoPass;
        plan_two_pass(B, R, L);
        return true;
    }
    if (plan_wave(P, R, Y, L)) { L.bwd = BwdRoute::Wave; return true; }
    Y.halves = Bwd1Layout::halves_for(P, npb);
    Y.dense_lanes = plan_dense_lanes(tb, P, Y, sw);
    const int64_t waves = (int64_t)R.row_tiles * Y.dim_slices * npb;
    Y.tiles_per_wave = (int)(waves >= 3 * 4096 ? waves / (2 * 4096) : 1);
    Y.row_groups = (R.row_tiles + kBwd1Waves * Y.tiles_per_wave - 1) / (kBwd1Waves * Y.tiles_per_wave);
    if (!Y.valid()) return false;
    L.bwd = BwdRoute::SinglePass;
    L.single = Y;
    L.dq_parts = npb;
    return true;
}

// Kernel configuration for a table shape: units per lane (vector width of the loads), waves per workgroup, the routes, and
// how many workgroups share a row tile / position tile so that the grid fills 256 CUs with 16-32 waves each.
static bool plan_pool(const mkb_tables_t *tb, int64_t B, int64_t P, const PoolSwitches &sw, PoolFolds folds, PoolPlan &L) {
    L = PoolPlan{};
    L.rel_elems = tb->n_relation * tb->relation_dim;
    L.rel_copies = plan_rel_copies(tb, B);
    L.n_entity = tb->n_entity;
    RowShape R;
    if (!plan_row_shape(tb, B, P, R, L)) return false;
    if (wants_matrix(tb, sw)) { plan_matrix(tb, B, P, R, sw, folds, L); return true; }
    plan_forward(tb, B, P, R, sw, L);
    return plan_backward(tb, B, P, R, sw, L);
}

}  // namespace mkb
