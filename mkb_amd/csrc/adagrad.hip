// mkb_adagrad_step: Adagrad with the element-wise semantics of torch.optim.Adagrad (weight_decay = 0, maximize = False), stepped
// ROW-SPARSELY and fused with optimizer.zero_grad():
//
//   sum += g * g ; p -= clr * g / (sqrt(sum) + eps) ; g = 0            clr = lr / (1 + (step - 1) * lr_decay), from the host
//
// An element whose gradient is zero keeps its p and its sum (the rule above is the identity there), so stepping only the rows a
// batch wrote IS dense Adagrad, bit for bit: there is nothing to defer, replay or flush (what most of adam.hip is about).  One
// launch per optimizer step: a 256-lane workgroup per listed row (6 streams of D floats: p, g, sum in; p, sum, zeroed g out), then
// the workgroups of the small dense tensors (relation table, pRotatE's modulus), then -- when a sampler lends its draw -- one
// workgroup that draws the next candidate pool (sampler_draw.h), exactly as the Adam launches carry it.
#include "common.h"
#include "sampler_draw.h"

#include <math.h>
#include <algorithm>

namespace mkb {

// One element.  Written once and used by every path (float4 rows, scalar rows, dense ranges): the listed form, the all-rows form
// and a de-duplicated id list give the same bits.  Nothing contracts: every operation rounds once, g * g included, which is what
// the kernels of torch.optim.Adagrad's foreach step do on this device (addcmul_ rounds the product before it adds: a fused
// g * g + sum differed from torch's accumulator in 13 - 16% of the elements of a step and in ~1.5% of the parameters, this form in
// none: tests/test_gpu_adagrad.py asserts torch.equal).  sqrtf and '/' are the correctly rounded ones (the build has no
// fast-math flags).  g == 0 (either sign): p and sum are left as loaded, not recomputed (0 / (sqrt(0) + 0) would be NaN).
__device__ __forceinline__ void adagrad_one(float &p, float g, float &s, float clr, float eps) {
#pragma clang fp contract(off)
    if (g != 0.f) {
        const float gg = g * g;
        s = s + gg;
        p = p - clr * g / (sqrtf(s) + eps);
    }
}

__device__ __forceinline__ void adagrad_four(float4 &p, const float4 &g, float4 &s, float clr, float eps) {
    adagrad_one(p.x, g.x, s.x, clr, eps);
    adagrad_one(p.y, g.y, s.y, clr, eps);
    adagrad_one(p.z, g.z, s.z, clr, eps);
    adagrad_one(p.w, g.w, s.w, clr, eps);
}

// A dense range (a small dense tensor, or the whole table in the all-rows form) over a grid-stride of 256-lane workgroups.
// vec: the three arrays are 16-byte aligned -> float4 body and a scalar tail; else scalar throughout.  A float4 whose four
// gradients are +0 is left alone altogether: the all-rows form reads a table's untouched rows and writes nothing.
__device__ __forceinline__ void adagrad_range(float *__restrict__ p, float *__restrict__ g, float *__restrict__ s, int64_t n, int vec,
                                              int64_t first, int64_t stride, float clr, float eps) {
    const int64_t n4 = vec ? (n >> 2) : 0;
    float4 *p4 = reinterpret_cast<float4 *>(p), *g4 = reinterpret_cast<float4 *>(g), *s4 = reinterpret_cast<float4 *>(s);
    for (int64_t i = first; i < n4; i += stride) {
        const float4 gg = g4[i];
        if ((__float_as_uint(gg.x) | __float_as_uint(gg.y) | __float_as_uint(gg.z) | __float_as_uint(gg.w)) == 0u) continue;
        float4 pp = p4[i], ss = s4[i];
        adagrad_four(pp, gg, ss, clr, eps);
        p4[i] = pp; s4[i] = ss; g4[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    for (int64_t i = (n4 << 2) + first; i < n; i += stride) {
        const float gg = g[i];
        if (__float_as_uint(gg) == 0u) continue;
        float pp = p[i], ss = s[i];
        adagrad_one(pp, gg, ss, clr, eps);
        p[i] = pp; s[i] = ss; g[i] = 0.f;
    }
}

constexpr int kAdagradDense = 8;              // dense tensors of one launch (mkb_adagrad_step: n_dense <= 8)
constexpr int kAdagradRanges = kAdagradDense + 1;  // ... and the whole table, in the all-rows form
constexpr int64_t kAdagradRangeBlocks = 2048;  // grid-stride workgroups per range, at most

struct AdagradArgs {
    float *p, *g, *s;
    int32_t *last;
    const int64_t *ids;   // listed form: the rows (duplicates allowed; entries outside [0, n_rows) are skipped)
    int64_t n_rows, D;
    int32_t step, n_row_blocks, vec4;  // vec4: rows are read as float4 (D % 4 == 0, 16-byte aligned arrays)
    float clr, eps;
    // the blocks behind the row blocks: range t owns [first_block[t], first_block[t + 1]), then the draw block
    float *rp[kAdagradRanges], *rg[kAdagradRanges], *rs[kAdagradRanges];
    int64_t rn[kAdagradRanges];
    int32_t rvec[kAdagradRanges], first_block[kAdagradRanges + 1];
    int32_t n_ranges;
    int32_t table_range;  // all-rows form: the range that is the table (its blocks also stamp `last`), else -1
    int32_t has_draw;     // the LAST block draws the negative sampler's next pool (pool_draw_body)
    DrawArgs draw;
};

__global__ __launch_bounds__(256) void adagrad_step_kernel(AdagradArgs A) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long lds_adagrad_draw[];  // only sized when a draw block rides
    __shared__ int s_old;
    const int bid = (int)blockIdx.x;
    if (bid >= A.n_row_blocks) {
        const int rb = bid - A.n_row_blocks;  // (workgroup-uniform from here on)
        if (A.has_draw && rb == A.first_block[A.n_ranges]) {
            pool_draw_body<256>(A.draw, lds_adagrad_draw);
            return;
        }
        int t = 0;
        while (t + 1 < A.n_ranges && rb >= A.first_block[t + 1]) ++t;
        const int64_t nb = A.first_block[t + 1] - A.first_block[t];
        const int64_t first = ((int64_t)rb - A.first_block[t]) * 256 + threadIdx.x, stride = nb * 256;
        adagrad_range(A.rp[t], A.rg[t], A.rs[t], A.rn[t], A.rvec[t], first, stride, A.clr, A.eps);
        if (t == A.table_range)
            for (int64_t r = first; r < A.n_rows; r += stride) A.last[r] = A.step;  // every row was visited by this step
        return;
    }
    const int64_t row = A.ids[bid];
    if (row < 0 || row >= A.n_rows) return;  // (workgroup-uniform) an id outside the table: skipped, not stepped out of bounds
    // exactly one workgroup owns a row: the first to stamp it with this step (steps are 1-based and strictly increasing)
    if (threadIdx.x == 0) s_old = atomicExch(&A.last[row], A.step);
    float *p = A.p + row * A.D, *g = A.g + row * A.D, *s = A.s + row * A.D;
    if (A.vec4) {
        float4 *p4 = reinterpret_cast<float4 *>(p), *g4 = reinterpret_cast<float4 *>(g), *s4 = reinterpret_cast<float4 *>(s);
        // the first float4s are requested BEFORE the ownership exchange returns (a global atomic round trip): a duplicate's
        // workgroup wastes three cached loads, every owner saves that latency
        const int64_t k0 = threadIdx.x, n4 = A.D >> 2;
        float4 pp0, gg0, ss0;
        if (k0 < n4) { pp0 = p4[k0]; gg0 = g4[k0]; ss0 = s4[k0]; }
        __syncthreads();
        if (s_old == A.step) return;  // duplicate id: another workgroup owns this row
        for (int64_t k = k0; k < n4; k += 256) {  // (rows longer than one float4 per lane: D = 2000 is 500 of them)
            float4 pp, gg, ss;
            if (k == k0) { pp = pp0; gg = gg0; ss = ss0; }
            else { pp = p4[k]; gg = g4[k]; ss = s4[k]; }
            adagrad_four(pp, gg, ss, A.clr, A.eps);
            p4[k] = pp; s4[k] = ss; g4[k] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
        return;
    }
    __syncthreads();
    if (s_old == A.step) return;
    for (int64_t k = threadIdx.x; k < A.D; k += 256) {
        float pp = p[k], ss = s[k];
        adagrad_one(pp, g[k], ss, A.clr, A.eps);
        p[k] = pp; s[k] = ss; g[k] = 0.f;
    }
}

static bool aligned16(const void *a, const void *b, const void *c) {
    return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c) & 15) == 0;
}

static void add_range(AdagradArgs &A, int &blocks, float *p, float *g, float *s, int64_t n) {
    const int t = A.n_ranges++;
    A.rp[t] = p; A.rg[t] = g; A.rs[t] = s; A.rn[t] = n;
    A.rvec[t] = aligned16(p, g, s) ? 1 : 0;
    A.first_block[t] = blocks;
    blocks += (int)std::min(std::max(((n >> 2) + 255) / 256, (int64_t)1), kAdagradRangeBlocks);
    A.first_block[t + 1] = blocks;
}

}  // namespace mkb

extern "C" int mkb_adagrad_step(float *param, float *grad, float *sum, int32_t *last, int64_t n_rows, int64_t D,
                                const int64_t *ids, int64_t n_ids, int64_t step, float clr, float eps,
                                const mkb_adagrad_dense_t *dense_host, int n_dense, mkb_sampler_t *draw_ahead, void *stream) {
    MKB_REQUIRE(n_dense >= 0 && n_dense <= mkb::kAdagradDense, "0..%d dense tensors, not %d", mkb::kAdagradDense, n_dense);
    MKB_REQUIRE(n_dense == 0 || dense_host, "dense tensors: null array");
    MKB_REQUIRE(step >= 1 && step < INT32_MAX, "bad step %lld (1-based)", (long long)step);
    MKB_REQUIRE(param || n_dense > 0, "nothing to step: no table and no dense tensor");
    mkb::AdagradArgs A{};
    A.clr = clr; A.eps = eps; A.step = (int32_t)step; A.table_range = -1;
    int blocks = 0;  // behind the row blocks
    for (int t = 0; t < n_dense; ++t) {
        const mkb_adagrad_dense_t &T = dense_host[t];
        MKB_REQUIRE(T.n >= 0 && (T.n == 0 || (T.param && T.grad && T.sum)), "dense tensor %d: null pointer or bad n", t);
    }
    if (param) {
        MKB_REQUIRE(grad && sum && last, "a table needs grad, sum and last");
        MKB_REQUIRE(D > 0 && n_rows >= 0 && n_rows < INT32_MAX, "bad D / n_rows (%lld, %lld)", (long long)D, (long long)n_rows);
        MKB_REQUIRE(n_ids >= 0 && n_ids <= INT32_MAX - 2 * mkb::kAdagradRanges * mkb::kAdagradRangeBlocks, "bad n_ids %lld", (long long)n_ids);
        MKB_REQUIRE(ids || n_ids == 0, "n_ids without ids");
        A.p = param; A.g = grad; A.s = sum; A.last = last; A.ids = ids; A.n_rows = n_rows; A.D = D;
        A.vec4 = ((D & 3) == 0 && mkb::aligned16(param, grad, sum)) ? 1 : 0;
        if (ids) A.n_row_blocks = (int32_t)n_ids;  // listed form: one workgroup per id
    }
    for (int t = 0; t < n_dense; ++t)
        if (dense_host[t].n > 0) mkb::add_range(A, blocks, dense_host[t].param, dense_host[t].grad, dense_host[t].sum, dense_host[t].n);
    if (param && !ids && n_rows > 0) {  // all-rows form: the table is one more dense range
        A.table_range = A.n_ranges;
        mkb::add_range(A, blocks, param, grad, sum, n_rows * D);
    }
    size_t lds = 0;
    if (draw_ahead && mkb::sampler_draw_ahead(draw_ahead, &A.draw, &lds)) { A.has_draw = 1; ++blocks; }
    if (A.n_row_blocks + blocks == 0) return MKB_OK;
    static mkb::LdsOptIn big_lds;
    if (int rc = big_lds.ensure(reinterpret_cast<const void *>(&mkb::adagrad_step_kernel), lds)) return rc;
    mkb::ProfScope ps(MKB_PROF_ADAM, (hipStream_t)stream);
    hipLaunchKernelGGL(mkb::adagrad_step_kernel, dim3((unsigned)(A.n_row_blocks + blocks)), dim3(256), lds, (hipStream_t)stream, A);
    MKB_LAUNCH_CHECK();
    return MKB_OK;
}
