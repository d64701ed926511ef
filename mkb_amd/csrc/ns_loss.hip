// mkb_ns_loss: margin ranking, pairwise logistic and sampled-softmax losses over one positive and K negatives per row,
// forward AND gradient seeds in one pass (include/mkb_hip.h, "negative-sampling loss family").
//
//   pairwise kinds, a_ij = param + neg_ij - pos_i:   row_i = sum_j p_ij f(a_ij),  f = max(0, a) (margin) or softplus(a)
//     p_ij = c_ij exp(alpha neg_ij) / sum_l c_il exp(alpha neg_il)  (detached, as in Adversarial; alpha = 0: c_ij / C_i)
//     dneg_ij = (w_i / W) p_ij f'(a_ij),  dpos_i = -sum_j dneg_ij
//   softmax, T = param:   row_i = log(exp(pos_i / T) + sum_j c_ij exp(neg_ij / T)) - pos_i / T
//     dneg_ij = (w_i / (W T)) c_ij exp(neg_ij / T) / Z_i,  dpos_i = -(w_i / (W T)) (Z_i - exp(pos_i / T)) / Z_i
//   loss = sum_i w_i row_i / W.
// c_ij: optional multiplicities (the pooled path: a column is a pool position).  A position with c_ij = 0 takes no part: its
// score is loaded but never enters an expression (it may be NaN), its seed is written as 0.
//
// The shape of loss.hip: one wave per row, four rows per 256-lane workgroup, W, the scratch and the finishing workgroup by the
// row-loss protocol of loss_math.h (RowLoss), per-row partials.  Rows of up to
// kNsStageCols columns are read from global memory once and kept in LDS ([row][column]: the 64 lanes of a column group hit 64
// consecutive words) for the three passes (max, partition sums, seeds); longer rows re-read global memory.  Every exponent is
// taken relative to the row maximum IN SCORE UNITS ((v - m) * scale): the subtraction is exact where it matters, and the
// softmax row is (m - pos) / T + log Z with no cancellation between two large terms.  No float atomics.
#include "common.h"
#include "loss_math.h"
#include "model_math.h"

namespace mkb {

constexpr int kNsStageCols = 1024;
constexpr int kNsRows = 4;  // rows (waves) per workgroup

template <int KIND>
__global__ __launch_bounds__(256) void ns_loss_rows_kernel(const float *__restrict__ pos, const float *__restrict__ neg,
                                                           const float *__restrict__ w, const uint16_t *__restrict__ cnt, int B,
                                                           int K, float param, float alpha, const float *__restrict__ scal,
                                                           float *__restrict__ scal_out, float *__restrict__ dpos,
                                                           float *__restrict__ dneg, float *__restrict__ rowpart) {
    constexpr bool SOFTMAX = KIND == MKB_LOSS_SOFTMAX;
    __shared__ float red[4];
    extern __shared__ float s_dyn[];
    const bool staged = K <= kNsStageCols;
    const int lane = threadIdx.x & 63, r = threadIdx.x >> 6;
    const int64_t i_raw = (int64_t)blockIdx.x * kNsRows + r;
    const int i = (int)min(i_raw, (int64_t)B - 1);  // (rows past the batch load row B-1 and leave after the workgroup-wide W reduction)
    const bool live = i_raw < B;
    float *s_v = s_dyn + (size_t)r * K;              // [kNsRows][K] scores (0 where the multiplicity is 0)
    float *s_e = s_dyn + (size_t)(kNsRows + r) * K;  // [kNsRows][K] multiplicities, then the softmax numerators
    const float wi = w ? w[i] : 1.f, p_i = pos[i];
    const float *nrow = neg + (int64_t)i * K;
    const uint16_t *crow = cnt ? cnt + (int64_t)i * K : nullptr;
    float *grow = dneg + (int64_t)i * K;

    float m = -INFINITY;
#pragma unroll 4
    for (int j = lane; j < K; j += 64) {
        const float c = crow ? (float)crow[j] : 1.f;
        const float raw = nrow[j];
        const float v = c > 0.f ? raw : 0.f;  // an unused position's score never enters an expression
        if (c > 0.f) m = fmaxf(m, v);
        if (staged) {
            s_v[j] = v;
            s_e[j] = c;
        }
    }
    const float W = row_loss_weight_sum(scal, scal_out, w, B, red);
    if (!live) return;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
    if (SOFTMAX) m = fmaxf(m, p_i);
    if (m == -INFINITY) m = 0.f;  // (a pairwise row that uses no position: every term below is masked)
    const float scale = SOFTMAX ? 1.f / param : alpha;

    auto f_of = [&](float a) { return KIND == MKB_LOSS_MARGIN ? fmaxf(a, 0.f) : -fast_log_sigmoid(-a); };
    auto df_of = [&](float a) { return KIND == MKB_LOSS_MARGIN ? (a > 0.f ? 1.f : 0.f) : fast_sigmoid(a); };

    float z = 0.f, s = 0.f;
#pragma unroll 2
    for (int j = lane; j < K; j += 64) {
        float c, v;
        if (staged) {
            c = s_e[j];
            v = s_v[j];
        } else {
            c = crow ? (float)crow[j] : 1.f;
            const float raw = nrow[j];
            v = c > 0.f ? raw : 0.f;
        }
        const float e = c > 0.f ? c * fast_exp((v - m) * scale) : 0.f;
        z += e;
        if (!SOFTMAX) s += e * f_of(param + v - p_i);
        if (staged) s_e[j] = e;
    }
    z = wave_sum(z);
    s = wave_sum(s);

    float coef, inv, gsum = 0.f, row, dp = 0.f;
    if (SOFTMAX) {
        const float Z = z + fast_exp((p_i - m) * scale);  // >= 1: the row maximum's own term is exp(0)
        inv = 1.f / Z;
        coef = wi * scale / W;
        row = (m - p_i) * scale + fast_log(Z);  // (no position used: m = pos, Z = 1, log2(1) = 0 exactly)
        dp = -coef * (z * inv);
    } else {
        inv = z > 0.f ? 1.f / z : 0.f;
        coef = wi / W;
        row = s * inv;
    }
#pragma unroll 2
    for (int j = lane; j < K; j += 64) {
        float e, v;
        if (staged) {
            e = s_e[j];
            v = s_v[j];
        } else {
            const float c = crow ? (float)crow[j] : 1.f;
            const float raw = nrow[j];
            v = c > 0.f ? raw : 0.f;
            e = c > 0.f ? c * fast_exp((v - m) * scale) : 0.f;
        }
        float g = 0.f;
        if (e > 0.f) g = SOFTMAX ? coef * (e * inv) : coef * (e * inv) * df_of(param + v - p_i);
        grow[j] = g;
        gsum += g;
    }
    if (!SOFTMAX) dp = -wave_sum(gsum);
    if (lane == 0) {
        dpos[i] = dp;
        rowpart[i] = wi * row;
    }
}

template <int KIND>
static void ns_loss_launch_rows(const float *pos, const float *neg, const float *weight, const uint16_t *cnt, int B, int K,
                                float param, float alpha, const RowLoss &L, float *dpos, float *dneg, hipStream_t st) {
    const size_t lds = K <= kNsStageCols ? (size_t)K * kNsRows * 2 * sizeof(float) : 0;  // <= 32 KB
    hipLaunchKernelGGL(ns_loss_rows_kernel<KIND>, dim3((unsigned)(((int64_t)B + kNsRows - 1) / kNsRows)), dim3(256), lds, st, pos,
                       neg, weight, cnt, B, K, param, alpha, L.scal_in, L.scal_out, dpos, dneg, L.rowpart);
}

}  // namespace mkb

using namespace mkb;

extern "C" int mkb_ns_loss(int kind, const float *pos, const float *neg, const float *weight, const uint16_t *cnt, int64_t B,
                           int64_t K, float param, float alpha, const float *weight_sum, float *loss, float *dpos, float *dneg,
                           float *scratch, void *stream) {
    MKB_REQUIRE(kind == MKB_LOSS_MARGIN || kind == MKB_LOSS_PAIR_LOGISTIC || kind == MKB_LOSS_SOFTMAX, "unknown loss kind %d", kind);
    MKB_REQUIRE(pos && neg && loss && dpos && dneg && scratch, "null pointer");
    MKB_REQUIRE(B >= 1 && K >= 1 && B <= INT32_MAX && K <= INT32_MAX && B * K <= INT32_MAX, "bad B / K (B * K <= 2^31 - 1)");
    MKB_REQUIRE(param - param == 0.f, "the margin / temperature must be finite");
    MKB_REQUIRE(alpha >= 0.f && alpha - alpha == 0.f, "alpha must be finite and >= 0");
    MKB_REQUIRE(kind != MKB_LOSS_SOFTMAX || param > 0.f, "the softmax temperature must be > 0");
    hipStream_t st = (hipStream_t)stream;
    ProfScope ps(MKB_PROF_LOSS, st);
    const RowLoss L = RowLoss::open(weight, weight_sum, B, scratch, st);
    switch (kind) {
        case MKB_LOSS_MARGIN:
            ns_loss_launch_rows<MKB_LOSS_MARGIN>(pos, neg, weight, cnt, (int)B, (int)K, param, alpha, L, dpos, dneg, st);
            break;
        case MKB_LOSS_PAIR_LOGISTIC:
            ns_loss_launch_rows<MKB_LOSS_PAIR_LOGISTIC>(pos, neg, weight, cnt, (int)B, (int)K, param, alpha, L, dpos, dneg, st);
            break;
        default:
            ns_loss_launch_rows<MKB_LOSS_SOFTMAX>(pos, neg, weight, cnt, (int)B, (int)K, param, alpha, L, dpos, dneg, st);
    }
    L.finish(B, 1.f, loss, st);
    MKB_LAUNCH_CHECK();
    return MKB_OK;
}
