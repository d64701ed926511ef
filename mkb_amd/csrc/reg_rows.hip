// mkb_reg_rows: the Lp (p = 2, 3) / N3 penalty on the embedding rows of a batch's positive triples, value AND gradient, written so
// that it touches only rows the training step touches anyway (include/mkb_hip.h, "embedding regularisers").
//
//   reg = sum_i (w_i / W) [lambda_e (f(E[h_i]) + f(E[t_i])) + lambda_r f(R[r_i])]
//   f(x) = sum_k |x_k|^p, or sum_{k < d} (re_k^2 + im_k^2)^(p / 2) for a table whose rows the model reads as [re | im] halves
//   (ComplEx: both tables; RotatE: the entity table).  For p = 2 the two forms are the same sum.
//
// The term of a row depends on that row alone, so the occurrences of a row collapse into a coefficient: c_row = sum of w_i / W over
// its occurrences, reg = sum over distinct rows of lambda c_row f(row), d reg / d row = lambda c_row f'(row).  The launches:
//   1. the 3 B occurrences (heads, tails, relations; relation keys follow the entity keys) radix-sorted by row in ONE sort
//      (pair_sort.h; the sort is stable: the occurrences of a row stay in batch order);
//   2. one 256-lane workgroup per sorted position; the one that opens a run owns the row, the others leave at once.  It sums the
//      run's weights (lane-strided partial sums in run order, then the fixed tree of block_sum_256), reads the row once with
//      16-byte loads where the dimension allows, adds lambda c f'(row) * scale to the gradient row -- a single writer per row, plain
//      vector stores, no atomics -- and writes the row's share of the value to its slot of `part` (0 for the other positions);
//   3. one workgroup sums the 3 B slots in a fixed order (the row losses' finish, loss_math.h, with c = 1 and no W).
// Nothing is accumulated with float atomics, so the value and both gradient tables have the same bits run to run, and a batch
// that puts every occurrence on one relation row (FB15k-237: ~4 per row at B = 1024; one relation: all B) costs one row write.
#include "common.h"
#include "loss_math.h"
#include "pair_sort.h"
#include "score_row.h"  // table_row

namespace mkb {

struct RegTable {
    const float *rows;
    float *grad;     // null: value only
    int64_t D;
    int d;           // half length when paired
    int paired;      // rows are [re | im] halves AND p = 3 (for p = 2 the element-wise form is the same sum)
    int vec4;        // 16-byte loads: the tables are 16-byte aligned, D (and d when paired) a multiple of 4
    float lambda;
};

struct RegArgs {
    RegTable ent, rel;
    const int *keys, *vals;   // the sorted occurrence list: row keys (relations: n_entity + r) and occurrence indices
    int n, B, n_entity;
    const float *w;           // [B] or null
    const float *scal;        // W on the device, or null: every workgroup reduces it from w (or takes B): RowLoss::scal_in
    const float *scale;       // upstream gradient on the device, or null = 1
    float *part;              // [n] or null (gradient only)
    int p;
};

// f and f' of one real entry
template <int P>
__device__ __forceinline__ void lp_real(float x, float &f, float &df) {
    if constexpr (P == 2) { f = x * x; df = 2.f * x; }
    else { const float a = fabsf(x); f = a * a * a; df = 3.f * x * a; }
}
// ... of one (re, im) pair for p = 3: f = m^3, f' = 3 m (re, im); m = 0 gives exactly 0
__device__ __forceinline__ void n3_pair(float re, float im, float &f, float &dre, float &dim) {
    const float m2 = re * re + im * im, m = sqrtf(m2);
    f = m2 * m;
    dre = 3.f * m * re;
    dim = 3.f * m * im;
}

// This lane's share of f(row); with a gradient row, g += cg f'(row) on the entries it owns.
template <int P>
__device__ __forceinline__ float reg_row_real(const float *__restrict__ x, float *__restrict__ g, int64_t D, bool vec4, float cg) {
    float s = 0.f;
    if (vec4) {
        for (int64_t k = (int64_t)threadIdx.x * 4; k < D; k += 1024) {
            const float4 v = *reinterpret_cast<const float4 *>(x + k);
            float4 f, df;
            lp_real<P>(v.x, f.x, df.x); lp_real<P>(v.y, f.y, df.y); lp_real<P>(v.z, f.z, df.z); lp_real<P>(v.w, f.w, df.w);
            s += (f.x + f.y) + (f.z + f.w);
            if (g) {
                float4 o = *reinterpret_cast<const float4 *>(g + k);
                o.x += cg * df.x; o.y += cg * df.y; o.z += cg * df.z; o.w += cg * df.w;
                *reinterpret_cast<float4 *>(g + k) = o;
            }
        }
    } else {
        for (int64_t k = threadIdx.x; k < D; k += 256) {
            float f, df;
            lp_real<P>(x[k], f, df);
            s += f;
            if (g) g[k] += cg * df;
        }
    }
    return s;
}

__device__ __forceinline__ float reg_row_paired(const float *__restrict__ x, float *__restrict__ g, int d, bool vec4, float cg) {
    float s = 0.f;
    if (vec4) {
        for (int k = (int)threadIdx.x * 4; k < d; k += 1024) {
            const float4 re = *reinterpret_cast<const float4 *>(x + k), im = *reinterpret_cast<const float4 *>(x + d + k);
            float4 f, dr, di;
            n3_pair(re.x, im.x, f.x, dr.x, di.x); n3_pair(re.y, im.y, f.y, dr.y, di.y);
            n3_pair(re.z, im.z, f.z, dr.z, di.z); n3_pair(re.w, im.w, f.w, dr.w, di.w);
            s += (f.x + f.y) + (f.z + f.w);
            if (g) {
                float4 a = *reinterpret_cast<const float4 *>(g + k), b = *reinterpret_cast<const float4 *>(g + d + k);
                a.x += cg * dr.x; a.y += cg * dr.y; a.z += cg * dr.z; a.w += cg * dr.w;
                b.x += cg * di.x; b.y += cg * di.y; b.z += cg * di.z; b.w += cg * di.w;
                *reinterpret_cast<float4 *>(g + k) = a;
                *reinterpret_cast<float4 *>(g + d + k) = b;
            }
        }
    } else {
        for (int k = threadIdx.x; k < d; k += 256) {
            float f, dr, di;
            n3_pair(x[k], x[d + k], f, dr, di);
            s += f;
            if (g) { g[k] += cg * dr; g[d + k] += cg * di; }
        }
    }
    return s;
}

__global__ __launch_bounds__(256) void reg_rows_kernel(RegArgs A) {
    __shared__ float red[4];
    const int pos = blockIdx.x;
    const int key = A.keys[pos];
    const bool is_rel = key >= A.n_entity;
    const RegTable &T = is_rel ? A.rel : A.ent;
    // (uniform across the workgroup) only the position that opens a run of equal keys owns the row
    if ((pos > 0 && A.keys[pos - 1] == key) || T.lambda == 0.f) {
        if (A.part && threadIdx.x == 0) A.part[pos] = 0.f;
        return;
    }
    // the run's weights: lane-strided in run order (a lane stops at the first key that is not the run's), then the fixed tree
    float acc = 0.f;
    for (int j = pos + (int)threadIdx.x; j < A.n && A.keys[j] == key; j += 256) acc += A.w ? A.w[A.vals[j] % A.B] : 1.f;
    const float W = row_loss_weight_sum(A.scal, A.w, A.B, red);  // (nothing to publish: the finish adds the slots up as they are)
    const float c = block_sum_256(acc, red) / W;
    const float cg = T.lambda * c * (A.scale ? A.scale[0] : 1.f);
    const int64_t row = is_rel ? key - A.n_entity : key;  // (a row of its table: the keys were clamped, pair_sort.hip)
    const float *x = T.rows + row * T.D;
    float *g = T.grad ? T.grad + row * T.D : nullptr;
    float s;
    if (T.paired) s = reg_row_paired(x, g, T.d, T.vec4 != 0, cg);
    else if (A.p == 2) s = reg_row_real<2>(x, g, T.D, T.vec4 != 0, cg);
    else s = reg_row_real<3>(x, g, T.D, T.vec4 != 0, cg);
    if (A.part) {  // (uniform)
        s = block_sum_256(s, red);
        if (threadIdx.x == 0) A.part[pos] = T.lambda * c * s;
    }
}

constexpr int64_t kRegMaxB = (int64_t)1 << 30;

struct RegPlan {
    PairSortPlan sort;
    size_t scal_off, part_off, total;
};

// B >= 1 is the caller's.  false: the shape is outside what one int32 sort covers (or the sort's size query failed: rc < 0)
static bool reg_plan(const mkb_tables_t *tb, int64_t B, RegPlan &P, int *rc) {
    *rc = 0;
    if (B >= kRegMaxB || 3 * B > INT32_MAX || tb->n_entity <= 0 || tb->n_relation <= 0 || tb->n_entity + tb->n_relation > INT32_MAX)
        return false;
    if ((*rc = pair_sort_plan(tb->n_entity + tb->n_relation, 3 * B, P.sort))) return false;
    P.scal_off = P.sort.total;
    P.part_off = P.scal_off + 256;
    P.total = P.part_off + (((size_t)3 * B * sizeof(float) + 255) & ~(size_t)255);
    return true;
}

static RegTable reg_table(const float *rows, float *grad, int64_t D, int d, bool halves, int p, float lambda) {
    RegTable t;
    t.rows = rows; t.grad = grad; t.D = D; t.d = d; t.lambda = lambda;
    t.paired = (halves && p == 3) ? 1 : 0;
    const bool aligned = ((((uintptr_t)rows) | ((uintptr_t)grad)) & 15) == 0;
    t.vec4 = (aligned && D % 4 == 0 && (!t.paired || d % 4 == 0)) ? 1 : 0;
    return t;
}

}  // namespace mkb

using namespace mkb;

extern "C" int64_t mkb_reg_rows_workspace_bytes(const mkb_tables_t *tb, int64_t B) {
    RegPlan P;
    int rc;
    if (!tb || B <= 0 || !reg_plan(tb, B, P, &rc)) return 0;
    return (int64_t)P.total;
}

extern "C" int mkb_reg_rows(const mkb_tables_t *tb, const mkb_grads_t *gr, const int64_t *sample, const float *weight, int64_t B, int p,
                            float lambda_ent, float lambda_rel, const float *weight_sum, const float *scale, float *value, void *ws,
                            int64_t ws_bytes, void *stream) {
    if (int rc = validate_tables(tb)) return rc;
    MKB_REQUIRE(p == 2 || p == 3, "p must be 2 or 3, not %d", p);
    MKB_REQUIRE(lambda_ent >= 0.f && lambda_ent - lambda_ent == 0.f && lambda_rel >= 0.f && lambda_rel - lambda_rel == 0.f,
                "the weights must be finite and >= 0");
    MKB_REQUIRE(sample != nullptr, "sample is null");
    MKB_REQUIRE(value != nullptr || gr != nullptr, "neither a value nor gradient buffers to write");
    MKB_REQUIRE(gr == nullptr || ((gr->g_ent || lambda_ent == 0.f) && (gr->g_rel || lambda_rel == 0.f)),
                "null gradient buffer of a table whose weight is not 0");
    MKB_REQUIRE(B >= 0 && B < kRegMaxB, "B must lie in [0, 2^30)");
    hipStream_t st = (hipStream_t)stream;
    if (B == 0) {
        if (value) MKB_CHECK_HIP(hipMemsetAsync(value, 0, sizeof(float), st));
        return MKB_OK;
    }
    RegPlan P;
    int rc;
    if (!reg_plan(tb, B, P, &rc)) {
        if (rc) return rc;  // (the sort's size query failed: its message stands)
        MKB_REQUIRE(false, "3 * B and n_entity + n_relation must stay below 2^31");
    }
    MKB_REQUIRE(ws != nullptr && (((uintptr_t)ws) & 255) == 0 && ws_bytes >= (int64_t)P.total, "workspace null, too small or unaligned");

    const int n = (int)(3 * B);
    PairKeySegs segs{};
    segs.seg[0] = PairKeySeg{sample, 3, B, tb->n_entity, 0};                        // heads
    segs.seg[1] = PairKeySeg{sample + 2, 3, B, tb->n_entity, 0};                    // tails
    segs.seg[2] = PairKeySeg{sample + 1, 3, B, tb->n_relation, (int)tb->n_entity};  // relations
    segs.n_segs = 3;
    RegArgs A;
    if (int rc2 = pair_sort_launch_segs(segs, ws, P.sort, st, &A.keys, &A.vals)) return rc2;
    const bool halves_e = tb->model == MKB_COMPLEX || tb->model == MKB_ROTATE, halves_r = tb->model == MKB_COMPLEX;
    A.ent = reg_table(tb->ent, gr ? gr->g_ent : nullptr, tb->entity_dim, tb->hidden_dim, halves_e, p, lambda_ent);
    A.rel = reg_table(tb->rel, gr ? gr->g_rel : nullptr, tb->relation_dim, tb->hidden_dim, halves_r, p, lambda_rel);
    A.n = n; A.B = (int)B; A.n_entity = (int)tb->n_entity;
    A.w = weight; A.scale = scale; A.p = p;
    A.part = value ? (float *)((unsigned char *)ws + P.part_off) : nullptr;
    // (W only: the value's slots are one per occurrence, in the workspace's own segment)
    A.scal = RowLoss::open(weight, weight_sum, B, (float *)((unsigned char *)ws + P.scal_off), st).scal_in;
    hipLaunchKernelGGL(reg_rows_kernel, dim3((unsigned)n), dim3(256), 0, st, A);
    if (value) hipLaunchKernelGGL(row_loss_finish_kernel, dim3(1), dim3(256), 0, st, A.part, n, 1.f, nullptr, value);
    MKB_LAUNCH_CHECK();
    return MKB_OK;
}
