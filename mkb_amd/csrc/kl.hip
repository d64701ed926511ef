// mkb_kl_divergence: distillation loss, forward AND both gradient seeds in one pass.
//
// Replaces losses.KlDivergence.__call__ (losses/kl_divergence.py:22-29):
//   loss = mean over ALL n*m entries of  F.kl_div(log_softmax(student / T, dim=1), softmax(teacher / T, dim=1), 'none')
//        = 1/(n m) * sum_i sum_j t_ij (log t_ij - log p_ij),     t = softmax(teacher / T), p = softmax(student / T)
//   (entries with t_ij == 0 contribute 0, as F.kl_div's xlogy does).  Closed-form gradients:
//   d loss / d student_ik = (p_ik - t_ik) / (n m T)
//   d loss / d teacher_ik = t_ik ((log t_ik - log p_ik) - KL_i) / (n m T),      KL_i = sum_j t_ij (log t_ij - log p_ij)
// The teacher gradient is not evaluated in that form: on a peaked teacher row (t_ir ~ 1) KL_i ~ log t_ir - log p_ir, and the
// difference of the two -- the row's largest gradient entry -- is left with the rounding error of KL_i, eps |KL_i|, however small
// it is itself (float32 torch autograd has the same cancellation).  With d_j = log t_ij - log p_ij and sum_j t_ij = 1,
//   d_k - KL_i = sum_j t_ij (d_k - d_j) = y_k - sum_j t_ij y_j,      y_j = d_j - d_r = (b_j - b_r) - (a_j - a_r),
// a = student / T, b = teacher / T, r = the row's first teacher maximum: y_r = 0 exactly, so the r-th entry is a plain sum of
// small terms, and every other entry carries the small factor t_ik.
// One wave per row (the distributions of distillation/distillation.py:486-558 hold a few entities / relations, m is small);
// correctly rounded expf / logf: this loss is compared with torch's CPU result at 1e-6.  Row partials are summed in a fixed
// order by a second single-workgroup launch, the row losses' finish (loss_math.h) with c = 1 / (n m) and no W: bit-reproducible.
#include "common.h"
#include "loss_math.h"
#include "model_math.h"

// No fused multiply-add in this file: the row maximum is taken over the rounded logits s * (1 / T), and `s * inv_T - max` as one
// fma would subtract it from the unrounded product and keep the rounding residual (see kl_rows_kernel).
#pragma clang fp contract(off)

namespace mkb {

__global__ __launch_bounds__(256) void kl_rows_kernel(const float *__restrict__ student, const float *__restrict__ teacher, int n,
                                                      int m, float inv_T, float *__restrict__ dstudent,
                                                      float *__restrict__ dteacher, float *__restrict__ rowpart) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n) return;
    const float *s = student + (int64_t)i * m, *t = teacher + (int64_t)i * m;
    // the logits a = s / T, b = t / T are rounded products (contraction is off), so a_j - max is exact and 0 at the maximum: one
    // candidate gives p = t = 1, loss and gradients 0.0, and y_r below is 0.0
    const auto a = [&](int j) { return s[j] * inv_T; };
    const auto b = [&](int j) { return t[j] * inv_T; };
    float ms = -INFINITY, mt = -INFINITY;
    for (int j = lane; j < m; j += 64) {
        ms = fmaxf(ms, a(j));
        mt = fmaxf(mt, b(j));
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        ms = fmaxf(ms, __shfl_xor(ms, off, 64));
        mt = fmaxf(mt, __shfl_xor(mt, off, 64));
    }
    float zs = 0.f, zt = 0.f;
    int r = m;
    for (int j = lane; j < m; j += 64) {
        zs += expf(a(j) - ms);
        zt += expf(b(j) - mt);
        if (r == m && b(j) == mt) r = j;
    }
    zs = wave_sum(zs);
    zt = wave_sum(zt);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) r = min(r, __shfl_xor(r, off, 64));
    if (r >= m) r = 0;  // (a row of NaN has no maximum: its gradients are NaN whichever entry is taken)
    const float ar = a(r);
    const float ls = logf(zs), lt = logf(zt);
    float kl = 0.f, ty = 0.f;
    for (int j = lane; j < m; j += 64) {
        const float logp = a(j) - ms - ls, logt = b(j) - mt - lt;
        const float tt = expf(logt);
        kl += tt > 0.f ? tt * (logt - logp) : 0.f;
        ty += tt > 0.f ? tt * ((b(j) - mt) - (a(j) - ar)) : 0.f;
    }
    kl = wave_sum(kl);
    ty = wave_sum(ty);
    const float c = inv_T / ((float)n * (float)m);
    for (int j = lane; j < m; j += 64) {
        const float logp = a(j) - ms - ls, logt = b(j) - mt - lt;
        const float pp = expf(logp), tt = expf(logt);
        dstudent[(int64_t)i * m + j] = c * (pp - tt);
        if (dteacher) dteacher[(int64_t)i * m + j] = tt > 0.f ? c * tt * (((b(j) - mt) - (a(j) - ar)) - ty) : 0.f;
    }
    if (lane == 0) rowpart[i] = kl;
}

}  // namespace mkb

using namespace mkb;

extern "C" int mkb_kl_divergence(const float *student, const float *teacher, int64_t n, int64_t m, float T, float *loss,
                                 float *dstudent, float *dteacher, float *scratch, void *stream) {
    MKB_REQUIRE(student && teacher && loss && dstudent && scratch, "null pointer");
    MKB_REQUIRE(n > 0 && m > 0 && n <= INT32_MAX && m <= INT32_MAX, "bad n / m");
    MKB_REQUIRE(T > 0.f, "temperature must be positive");
    hipStream_t st = (hipStream_t)stream;
    ProfScope ps(MKB_PROF_LOSS, st);
    hipLaunchKernelGGL(kl_rows_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, student, teacher, (int)n, (int)m, 1.f / T,
                       dstudent, dteacher, scratch);
    hipLaunchKernelGGL(row_loss_finish_kernel, dim3(1), dim3(256), 0, st, scratch, (int)n, 1.f / ((float)n * (float)m), nullptr, loss);
    MKB_LAUNCH_CHECK();
    return MKB_OK;
}
