// Triple classification (evaluation/classif.py; reference evaluation/classif.py:89-155): the threshold that maximises
// tpr - fpr over the ROC points sklearn.metrics.roc_curve keeps, per group, and the accuracy count at given thresholds.
// Integer counts, an integer max and two IEEE double divisions per candidate only: no float atomics, no sort; every result
// is bit-identical from run to run and does not depend on the launch shape.
//
// Scores are compared through ordered_bits(): the int32 whose order is the order of the finite floats, with -0.0 and +0.0
// on the same value.  Integer compares do not depend on the denormal mode.
#include "common.h"

namespace mkb {

constexpr int kClsThreads = 256;
constexpr int kOrdNone = INT32_MIN;  // "no score below this one" (below ordered_bits of every float)
constexpr int kOrdInf = 0x7f800000;  // ordered_bits(+inf): above every finite score

__device__ __forceinline__ int ordered_bits(float x) {
    const int b = __float_as_int(x);
    return b >= 0 ? b : (int)(0x80000000u - (unsigned)b);
}
__device__ __forceinline__ bool is_finite_bits(float x) { return (__float_as_int(x) & 0x7fffffff) < 0x7f800000; }

// Workspace of one search, n items (9 int32 per item, each array n long):
//   ord   ordered_bits of the score
//   key   2 * group + (label > 0) for an item that takes part; -1: in no group; -2 - group: in a group, score not finite
//   tp_ge fp_ge tp_gt fp_gt   positives / negatives of the item's group with a score >= / > the item's
//   nxt   the largest ord below the item's among its group (kOrdNone: there is none)
//   tp_eq fp_eq   positives / negatives of the item's group with a score == nxt
// The counts and nxt are gathered with integer atomics (add, max) by the workgroups that share an item's pairs: the result
// does not depend on their order.
struct SearchWs {
    int *ord, *key;
    unsigned *tp_ge, *fp_ge, *tp_gt, *fp_gt;
    int *nxt;
    unsigned *tp_eq, *fp_eq;
};
constexpr int kSearchWsWords = 9;

__host__ inline SearchWs search_ws(void *ws, int64_t n) {
    int *p = static_cast<int *>(ws);
    SearchWs w;
    w.ord = p, w.key = p + n;
    w.tp_ge = reinterpret_cast<unsigned *>(p + 2 * n), w.fp_ge = reinterpret_cast<unsigned *>(p + 3 * n);
    w.tp_gt = reinterpret_cast<unsigned *>(p + 4 * n), w.fp_gt = reinterpret_cast<unsigned *>(p + 5 * n);
    w.nxt = p + 6 * n;
    w.tp_eq = reinterpret_cast<unsigned *>(p + 7 * n), w.fp_eq = reinterpret_cast<unsigned *>(p + 8 * n);
    return w;
}

__global__ __launch_bounds__(kClsThreads) void search_keys_kernel(const float *__restrict__ score, const int64_t *__restrict__ label,
                                                                  const int32_t *__restrict__ group, int64_t n, int n_groups,
                                                                  SearchWs w) {
    const int64_t i = (int64_t)blockIdx.x * kClsThreads + threadIdx.x;
    if (i >= n) return;
    const float s = score[i];
    const int g = group ? group[i] : 0;
    int key = -1;
    if (g >= 0 && g < n_groups) key = is_finite_bits(s) ? 2 * g + (label[i] > 0 ? 1 : 0) : -2 - g;
    w.ord[i] = ordered_bits(s);
    w.key[i] = key;
    w.tp_ge[i] = w.fp_ge[i] = w.tp_gt[i] = w.fp_gt[i] = w.tp_eq[i] = w.fp_eq[i] = 0u;
    w.nxt[i] = kOrdNone;
}

// The pair passes run on a (items / 256) x (splits) grid: workgroup (x, y) meets the 256 items of tile x with the tiles
// [tiles * y / splits, tiles * (y + 1) / splits) of all items.  A few thousand items alone give too few workgroups of 256 lanes
// to fill the device: the splits bring the grid to about four workgroups per compute unit.
__device__ __forceinline__ void pair_range(int64_t n, int64_t &j_lo, int64_t &j_hi) {
    const int64_t tiles = (n + kClsThreads - 1) / kClsThreads;
    j_lo = tiles * blockIdx.y / gridDim.y * kClsThreads;
    j_hi = min(n, tiles * (blockIdx.y + 1) / gridDim.y * kClsThreads);
}

// Stages items j0 .. j0 + 255 (ord, key) in LDS; past the end: a key nobody matches.
__device__ __forceinline__ void stage_tile(const SearchWs &w, int64_t j0, int64_t n, int2 *s_tile) {
    const int64_t j = j0 + threadIdx.x;
    s_tile[threadIdx.x] = j < n ? make_int2(w.ord[j], w.key[j]) : make_int2(0, -1);
}

// Pass A: lane = item i; over the items j of this workgroup's range that are of the same group (tiles of 256 staged in LDS,
// every lane reads the same address: a broadcast): the four counts and nxt.  An item that takes no part (key < 0) matches
// nobody.
__global__ __launch_bounds__(kClsThreads) void search_count_kernel(int64_t n, SearchWs w) {
    __shared__ int2 s_tile[kClsThreads];
    const int64_t i = (int64_t)blockIdx.x * kClsThreads + threadIdx.x;
    const int key = i < n ? w.key[i] : -1;
    const int v = i < n ? w.ord[i] : 0;
    // a staged key is compared only with non-negative values or INT32_MIN + 1 / + 2, which no staged key takes
    const int kpos = key >= 0 ? (key | 1) : INT32_MIN + 1, kneg = key >= 0 ? (key & ~1) : INT32_MIN + 2;
    unsigned tp_ge = 0, fp_ge = 0, tp_gt = 0, fp_gt = 0;
    int nxt = kOrdNone;
    int64_t j_lo, j_hi;
    pair_range(n, j_lo, j_hi);
    for (int64_t j0 = j_lo; j0 < j_hi; j0 += kClsThreads) {
        __syncthreads();
        stage_tile(w, j0, n, s_tile);
        __syncthreads();
#pragma unroll 8
        for (int jj = 0; jj < kClsThreads; ++jj) {
            const int2 t = s_tile[jj];
            const bool p = t.y == kpos, q = t.y == kneg, ge = t.x >= v, gt = t.x > v;
            tp_ge += p && ge, fp_ge += q && ge, tp_gt += p && gt, fp_gt += q && gt;
            if ((p || q) && !ge) nxt = max(nxt, t.x);
        }
    }
    if (i >= n || key < 0) return;
    if (tp_ge) atomicAdd(&w.tp_ge[i], tp_ge);
    if (fp_ge) atomicAdd(&w.fp_ge[i], fp_ge);
    if (tp_gt) atomicAdd(&w.tp_gt[i], tp_gt);
    if (fp_gt) atomicAdd(&w.fp_gt[i], fp_gt);
    if (nxt != kOrdNone) atomicMax(&w.nxt[i], nxt);
}

// Pass B (after pass A is complete): the positives / negatives of the item's group at score == nxt.
__global__ __launch_bounds__(kClsThreads) void search_next_kernel(int64_t n, SearchWs w) {
    __shared__ int2 s_tile[kClsThreads];
    const int64_t i = (int64_t)blockIdx.x * kClsThreads + threadIdx.x;
    const int key = i < n ? w.key[i] : -1;
    const int nxt = i < n ? w.nxt[i] : kOrdNone;
    const int kpos = key >= 0 ? (key | 1) : INT32_MIN + 1, kneg = key >= 0 ? (key & ~1) : INT32_MIN + 2;
    unsigned tp_eq = 0, fp_eq = 0;
    int64_t j_lo, j_hi;
    pair_range(n, j_lo, j_hi);
    for (int64_t j0 = j_lo; j0 < j_hi; j0 += kClsThreads) {
        __syncthreads();
        stage_tile(w, j0, n, s_tile);
        __syncthreads();
#pragma unroll 8
        for (int jj = 0; jj < kClsThreads; ++jj) {
            const int2 t = s_tile[jj];
            const bool eq = t.x == nxt;
            tp_eq += eq && t.y == kpos, fp_eq += eq && t.y == kneg;
        }
    }
    if (i >= n || key < 0) return;
    if (tp_eq) atomicAdd(&w.tp_eq[i], tp_eq);
    if (fp_eq) atomicAdd(&w.fp_eq[i], fp_eq);
}

// roc_curve's keep rule for the score of item i: the first and the last distinct score, and every score at which the second
// difference of tps or fps (in descending score order) is not zero.
__device__ __forceinline__ bool is_curve_point(const SearchWs &w, int64_t i) {
    const int64_t tp_ge = w.tp_ge[i], fp_ge = w.fp_ge[i], tp_gt = w.tp_gt[i], fp_gt = w.fp_gt[i];
    const int64_t tp_nx = tp_ge + w.tp_eq[i], fp_nx = fp_ge + w.fp_eq[i];
    const bool highest = tp_gt + fp_gt == 0, lowest = w.nxt[i] == kOrdNone;
    return highest || lowest || tp_nx - 2 * tp_ge + tp_gt != 0 || fp_nx - 2 * fp_ge + fp_gt != 0;
}

// One candidate of the selection: J = tpr - fpr in double, then the score (through its ord; kOrdInf + 1 for the extra first
// point of roc_curve, threshold +inf, J 0.0).  `better` is the strict lexicographic order: roc_curve lists the points by
// descending threshold and numpy's argmax takes the first maximum.
struct Pick {
    double J;
    int ord;
    float score;
    unsigned tp, fp;
};
__device__ __forceinline__ bool better(const Pick &a, const Pick &b) { return a.J > b.J || (a.J == b.J && a.ord > b.ord); }

// Workgroup g: the totals of group g, then the best kept item.  Lane l takes items l, l + 256, ... in that order and the 256
// candidates meet pairwise in LDS (stride 128, 64, ..., 1): the order is a function of n alone.
__global__ __launch_bounds__(kClsThreads) void search_select_kernel(const float *__restrict__ score, int64_t n, SearchWs w,
                                                                    float *__restrict__ threshold, int64_t *__restrict__ stats) {
    __shared__ unsigned s_cnt[4][kClsThreads];
    __shared__ Pick s_pick[kClsThreads];
    const int g = (int)blockIdx.x, lane = (int)threadIdx.x;
    unsigned P = 0, N = 0, bad = 0, items = 0;
    for (int64_t i = lane; i < n; i += kClsThreads) {
        const int key = w.key[i];
        if (key >= 0 && (key >> 1) == g) P += key & 1, N += !(key & 1), items += 1;
        else if (key == -2 - g) bad += 1, items += 1;
    }
    s_cnt[0][lane] = P, s_cnt[1][lane] = N, s_cnt[2][lane] = bad, s_cnt[3][lane] = items;
    __syncthreads();
    for (int off = kClsThreads / 2; off > 0; off >>= 1) {
        if (lane < off) {
#pragma unroll
            for (int c = 0; c < 4; ++c) s_cnt[c][lane] += s_cnt[c][lane + off];
        }
        __syncthreads();
    }
    P = s_cnt[0][0], N = s_cnt[1][0], bad = s_cnt[2][0], items = s_cnt[3][0];
    Pick best{0.0, kOrdInf + 1, __int_as_float(kOrdInf), 0u, 0u};
    if (P > 0 && N > 0) {
        for (int64_t i = lane; i < n; i += kClsThreads) {
            const int key = w.key[i];
            if (key < 0 || (key >> 1) != g || !is_curve_point(w, i)) continue;
            const unsigned tp = w.tp_ge[i], fp = w.fp_ge[i];
            // two correctly rounded double divisions and one subtraction, as numpy computes tps / tps[-1] - fps / fps[-1]
            const double tpr = (double)tp / (double)P, fpr = (double)fp / (double)N;
            const Pick cand{tpr - fpr, w.ord[i], score[i], tp, fp};
            if (better(cand, best)) best = cand;
        }
    }
    s_pick[lane] = best;
    __syncthreads();
    for (int off = kClsThreads / 2; off > 0; off >>= 1) {
        if (lane < off && better(s_pick[lane + off], s_pick[lane])) s_pick[lane] = s_pick[lane + off];
        __syncthreads();
    }
    if (lane == 0) {
        const Pick top = s_pick[0];
        threshold[g] = top.score;
        int64_t *out = stats + 6 * (int64_t)g;
        out[0] = P, out[1] = N, out[2] = top.tp, out[3] = top.fp, out[4] = bad, out[5] = items;
    }
}

// Workgroup g counts the items of group g and those the threshold of g classifies correctly: score >= threshold and
// label > 0, or score < threshold and label <= 0.  A NaN score (or threshold) is neither: the item counts as wrong.
__global__ __launch_bounds__(kClsThreads) void threshold_accuracy_kernel(const float *__restrict__ score, const int64_t *__restrict__ label,
                                                                         const int32_t *__restrict__ group, int64_t n,
                                                                         const float *__restrict__ threshold,
                                                                         int64_t *__restrict__ counts) {
    __shared__ int64_t s_cnt[2][kClsThreads];
    const int g = (int)blockIdx.x, lane = (int)threadIdx.x;
    const float thr = threshold[g];
    const bool thr_nan = (__float_as_int(thr) & 0x7fffffff) > 0x7f800000;
    const int t = ordered_bits(thr);
    int64_t correct = 0, items = 0;
    for (int64_t i = lane; i < n; i += kClsThreads) {
        if ((group ? group[i] : 0) != g) continue;
        items += 1;
        const float s = score[i];
        if (thr_nan || (__float_as_int(s) & 0x7fffffff) > 0x7f800000) continue;
        correct += (ordered_bits(s) >= t) == (label[i] > 0);
    }
    s_cnt[0][lane] = correct, s_cnt[1][lane] = items;
    __syncthreads();
    for (int off = kClsThreads / 2; off > 0; off >>= 1) {
        if (lane < off) s_cnt[0][lane] += s_cnt[0][lane + off], s_cnt[1][lane] += s_cnt[1][lane + off];
        __syncthreads();
    }
    if (lane < 2) counts[2 * (int64_t)g + lane] = s_cnt[lane][0];
}

constexpr unsigned kPairWorkgroups = 1024;  // the pair passes' grid is split until it has about this many workgroups
constexpr int kMaxGroups = 1 << 24;  // 2 * group + 1 and -2 - group stay int32; one workgroup per group
// The selection and the accuracy count launch one workgroup per group, and each strides over all n items: n_groups * n item
// visits.  That suits a few hundred relations; the bound (seconds of work) keeps a mistaken group count from hanging a device.
constexpr int64_t kMaxGroupItemVisits = (int64_t)1 << 32;

}  // namespace mkb

extern "C" int64_t mkb_threshold_search_workspace_bytes(int64_t n, int n_groups) {
    if (n < 0 || n > MKB_THRESHOLD_SEARCH_MAX_N || n_groups <= 0) return -1;
    return mkb::kSearchWsWords * n * (int64_t)sizeof(int32_t);
}

extern "C" int mkb_threshold_search(const float *score, const int64_t *label, const int32_t *group, int64_t n, int n_groups,
                                    float *threshold, int64_t *stats, void *ws, int64_t ws_bytes, void *stream) {
    MKB_REQUIRE(n >= 0 && n_groups > 0 && n_groups <= mkb::kMaxGroups, "bad size (%lld items, %d groups)", (long long)n, n_groups);
    MKB_REQUIRE(n <= MKB_THRESHOLD_SEARCH_MAX_N,
                "%lld items are above the cap of the all-pairs threshold search (%lld): search on the host instead", (long long)n,
                (long long)MKB_THRESHOLD_SEARCH_MAX_N);
    MKB_REQUIRE((int64_t)n_groups * n <= mkb::kMaxGroupItemVisits, "%d groups x %lld items: every group's workgroup visits every item",
                n_groups, (long long)n);
    MKB_REQUIRE(threshold && stats && ((score && label) || n == 0), "null pointer");
    const int64_t need = mkb_threshold_search_workspace_bytes(n, n_groups);
    MKB_REQUIRE(n == 0 || (ws && ws_bytes >= need && (uintptr_t)ws % 4 == 0), "workspace: %lld bytes given, %lld needed (4-byte aligned)",
                (long long)ws_bytes, (long long)need);
    hipStream_t st = (hipStream_t)stream;
    const mkb::SearchWs w = mkb::search_ws(ws, n);
    if (n > 0) {
        const unsigned blocks = (unsigned)((n + mkb::kClsThreads - 1) / mkb::kClsThreads);
        hipLaunchKernelGGL(mkb::search_keys_kernel, dim3(blocks), dim3(mkb::kClsThreads), 0, st, score, label, group, n, n_groups, w);
        const unsigned want = (mkb::kPairWorkgroups + blocks - 1) / blocks;
        const dim3 grid(blocks, want < blocks ? want : blocks);
        hipLaunchKernelGGL(mkb::search_count_kernel, grid, dim3(mkb::kClsThreads), 0, st, n, w);
        hipLaunchKernelGGL(mkb::search_next_kernel, grid, dim3(mkb::kClsThreads), 0, st, n, w);
    }
    hipLaunchKernelGGL(mkb::search_select_kernel, dim3((unsigned)n_groups), dim3(mkb::kClsThreads), 0, st, score, n, w, threshold, stats);
    MKB_LAUNCH_CHECK();
    return MKB_OK;
}

extern "C" int mkb_threshold_accuracy(const float *score, const int64_t *label, const int32_t *group, int64_t n, const float *threshold,
                                      int n_groups, int64_t *counts, void *stream) {
    MKB_REQUIRE(n >= 0 && n <= INT64_MAX / 4 && n_groups > 0 && n_groups <= mkb::kMaxGroups, "bad size (%lld items, %d groups)",
                (long long)n, n_groups);
    MKB_REQUIRE(n == 0 || n_groups <= mkb::kMaxGroupItemVisits / n, "%d groups x %lld items: every group's workgroup visits every item",
                n_groups, (long long)n);
    MKB_REQUIRE(threshold && counts && ((score && label) || n == 0), "null pointer");
    hipLaunchKernelGGL(mkb::threshold_accuracy_kernel, dim3((unsigned)n_groups), dim3(mkb::kClsThreads), 0, (hipStream_t)stream, score,
                       label, group, n, threshold, counts);
    MKB_LAUNCH_CHECK();
    return MKB_OK;
}
