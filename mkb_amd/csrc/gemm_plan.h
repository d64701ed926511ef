// Launch plan of one matrix-core product (gemm_mfma.h): which kernel family runs, with which tiles, K split, grid and dynamic
// LDS, where C goes, which tail is pending and how many floats the product writes into the partial buffer.  plan_gemm is
// the ONE place these are decided: the launchers of gemm_mfma.h launch from a GemmPlan, and the callers size their buffers from
// it (score_pool.hip: PoolPlan and carve; rank.hip).  Plain host code: no device code, no HIP calls, no environment.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace mkb {

// GEMM_ACCUM: C += A . B, every element of C written by exactly one tile (a K split goes through the partial buffer and a
// fixed-order reduction that adds the finished product once): the dense entity gradient of the 1vsAll step (score_all.hip)
enum { GEMM_STORE = 0, GEMM_STORE_AFFINE = 1, GEMM_ATOMIC_ROWS = 2, GEMM_ACCUM = 3 };
constexpr int kBfPitch = 80;  // bytes between rows of a bf16 plane (the staging of the bf16x3 kernels)
constexpr size_t kGemmLdsMax = 160 * 1024;  // LDS of a CU: a plan that asks for more cannot launch

// The per-call switches of the products (DESIGN.md "Run-time switches"), read once per ABI call by the caller
struct GemmSwitches {
    bool no128;    // MKB_GEMM_NO128 set: never the 128-row tiles
    bool no_pair;  // MKB_GEMM_NO_PAIR set: the two backward products as two launches
    bool bf16x3;   // MKB_GEMM_BF16X3 (default 1): the 128-row tiles split fp32 three ways on the bf16 pipe; 0: the fp32-input instruction
};

// What the decisions read of a product C [M, N] = A [M, K] . B [K, N]
struct GemmShape {
    int M, N, K;
    int64_t lda, ldb, ldc;
    bool a_mk, b_nk;  // operand layouts (gemm_mfma.h): A k-contiguous / B k-contiguous
    int epi;          // GEMM_STORE, GEMM_STORE_AFFINE, GEMM_ATOMIC_ROWS
    bool aligned16;   // both operand base pointers are 16-byte aligned
    int64_t b_rows;   // rows of the table B addresses: of the gathered table (0 = unknown), else N (b_nk) or K
};

// What the caller allows
struct GemmLimits {
    bool partials;   // a partial buffer exists; it must hold GemmPlan::part_floats floats
    int slices_cap;  // > 0 (GEMM_STORE): C is [slices][M][ldc] and the caller's consumer adds up to slices_cap partial products itself
    int want_wg;     // workgroups wanted of the 128-row tiles (0: ~1 per CU)
    int max_ks;      // the largest K split (1: a caller with room for ONE C and no partial buffer -- the ranking route)
    bool fold_tail;  // the caller folds a pending tail into its next launch (GemmTail, common.h) instead of having it launched
};

enum class GemmKernel { F32Tile64, F32Tile128, Bf16x3Tile128 };  // gemm_f32_mfma_kernel / gemm128_f32_mfma_kernel / gemm128_bf16x3_*
enum class GemmDest { Final, Partials, Slices };                 // C itself / [ks][M][ld] in the partial buffer / the caller's slices
enum class GemmTailKind { None = 0, Reduce = 1, Scatter = 2 };   // (the values are GemmTail's kinds)

struct GemmPlan {
    GemmShape s;
    GemmKernel kernel;
    int tm, tn, ks;      // tile (tm 32: the 64-row kernel with two waves), K split
    unsigned mx, ny;     // grid (mx, ny, ks)
    unsigned wg;         // lanes per workgroup
    size_t lds;          // dynamic LDS bytes
    GemmDest dest;
    GemmTailKind tail;   // Reduce: C = c0 + c1 * sum of the partials; Scatter: C[c_idx[m]] += sum of the partials [ks][M][N]
    bool tail_handed;    // the tail is described to the caller (fold_tail and the 128-row tiles), else launched behind the product
    size_t part_floats;  // floats written into the partial buffer
    // ... and the most any plan of this product writes there, whatever the switches, the workgroups wanted and the slices:
    // max_ks partial products.  Callers that cache a buffer across switch settings size it by this.
    size_t part_bound;

    int slices() const { return dest == GemmDest::Slices ? ks : 1; }  // [M][ldc] partial products the caller's consumer adds up
    unsigned blocks() const { return mx * ny * (unsigned)ks; }
};

// These products are small (1-2 GFLOP) and short in one dimension: fill the chip by narrowing / halving the tile and / or
// splitting K.  A K split needs somewhere to put its partial products: the partial buffer (a fixed-order reduction or the
// scattered add follows: the tail), the caller's slices, or -- 64-row tiles only -- the atomic epilogue, which just accumulates.
inline GemmPlan plan_gemm(const GemmShape &s, const GemmLimits &lim, const GemmSwitches &sw) {
    GemmPlan p{};
    p.s = s;
    p.part_bound = lim.partials ? (size_t)lim.max_ks * s.M * (s.epi == GEMM_ATOMIC_ROWS ? (size_t)s.N : (size_t)s.ldc) : 0;
    const bool to_slices = lim.slices_cap > 0 && s.epi == GEMM_STORE;
    const bool atomic = s.epi == GEMM_ATOMIC_ROWS;
    auto split = [&](int tiles, int want, int min_k) {
        int ks = 1;
        while (tiles * ks < want && ks < lim.max_ks && s.K / (ks * 2) >= min_k && (!to_slices || ks * 2 <= lim.slices_cap)) ks *= 2;
        return ks;
    };
    auto chunk_ids = [&](int ks) { return (size_t)(((s.K + ks - 1) / ks + 31) / 32 * 32) * 4; };  // row ids of a K range
    // 128 x 128 / 128 x 64 tiles (4 / 2 accumulators per wave) when the operands allow 16-byte loads
    // The bf16x3 kernel's buffer loads address an operand with SIGNED 32-bit byte offsets: every row it can touch must lie
    // within 2 GB of the base; larger operands take the fp32 kernel
    const int64_t a_span = (s.a_mk ? (int64_t)s.M * s.lda : (int64_t)s.K * s.lda) * 4;
    const bool fits32 = a_span < ((int64_t)1 << 31) && s.b_rows > 0 && s.b_rows * s.ldb * 4 < ((int64_t)1 << 31);
    const bool bf = sw.bf16x3 && fits32;
    // M % 4: the fp32 tiles load an m-contiguous A four rows at a time.  The bf16x3 kernel loads it one value per lane and every
    // kernel stores C element by element, so the accumulating product -- M is the entity count, whatever that is -- keeps the
    // 128-row tiles there
    const bool m_ok = s.M % 4 == 0 || (s.epi == GEMM_ACCUM && !s.a_mk && bf);
    const bool al = s.aligned16 && s.lda % 4 == 0 && s.ldb % 4 == 0 && m_ok && s.N % 4 == 0 && s.K % 4 == 0;
    const int m128 = (s.M + 127) / 128, tiles128 = m128 * ((s.N + 127) / 128);
    bool big = !sw.no128 && al && tiles128 >= 24 && (lim.partials || lim.max_ks <= 1);
    if (big) {
        // fill ~256 CUs: prefer the narrower tile (no K split, no reduction launch) to splitting K
        p.tn = tiles128 < 200 ? 64 : 128;
        p.tm = 128;
        p.mx = (unsigned)m128; p.ny = (unsigned)((s.N + p.tn - 1) / p.tn);
        p.wg = 256;
        // workgroups wanted: ~1 per CU by default; the products whose tail rides the next launch ask for 2 (want_wg = 500: a lone
        // 4-wave workgroup leaves each SIMD's matrix pipe idle during its staging; measured 37 -> 29 us)
        p.ks = split((int)(p.mx * p.ny), lim.want_wg ? lim.want_wg : 200, 96);
        p.kernel = bf ? GemmKernel::Bf16x3Tile128 : GemmKernel::F32Tile128;
        // (two stages of a 128 x 128 fp32 tile pair are 66 KB: more than the 64 KB a kernel gets without asking)
        p.lds = (p.kernel == GemmKernel::Bf16x3Tile128 ? (size_t)3 * (128 + p.tn) * kBfPitch : (size_t)2 * (128 + p.tn) * 33 * 4) + chunk_ids(p.ks);
        // the scattered product always goes through partials [ks][M][N] and ONE atomic per element
        p.tail = atomic ? GemmTailKind::Scatter : (p.ks > 1 && !to_slices ? GemmTailKind::Reduce : GemmTailKind::None);
        p.tail_handed = lim.fold_tail && p.tail != GemmTailKind::None;
        // the row ids of a K range are staged whole: a K of hundreds of thousands (every entity of a large graph) does not fit
        if (p.lds > kGemmLdsMax) {
            big = false;
            p.lds = 0;
            p.tail_handed = false;
        }
    }
    if (!big) {
        const int n64 = (s.N + 63) / 64, tiles64 = ((s.M + 63) / 64) * n64;
        p.tm = tiles64 < 256 ? 32 : 64;  // few tiles: two waves per workgroup, twice the workgroups
        p.tn = 64;
        p.kernel = GemmKernel::F32Tile64;
        p.mx = (unsigned)((s.M + p.tm - 1) / p.tm); p.ny = (unsigned)n64;
        p.wg = (unsigned)p.tm * 4;
        p.ks = atomic || lim.partials || to_slices ? split((int)(p.mx * p.ny), 768, 128) : 1;
        p.tail = p.ks > 1 && !atomic && !to_slices ? GemmTailKind::Reduce : GemmTailKind::None;
    }
    p.dest = to_slices ? GemmDest::Slices : (p.tail != GemmTailKind::None ? GemmDest::Partials : GemmDest::Final);
    if (p.dest == GemmDest::Partials) p.part_floats = (size_t)p.ks * s.M * (p.tail == GemmTailKind::Scatter ? (size_t)s.N : (size_t)s.ldc);
    return p;
}

}  // namespace mkb
