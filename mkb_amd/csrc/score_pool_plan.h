// Launch plan of the pooled scoring path: which kernel runs for a table shape, with which grid, over which workspace
// layout.  score_pool.hip fills a PoolPlan (plan_pool) and carves the workspace from it; score_pool_launch.h launches the VALU
// routes from it, gemm_mfma.h the matrix route's three products (their GemmPlans, gemm_plan.h, are part of the plan).
#pragma once
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

}  // namespace mkb
