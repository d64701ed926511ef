// Device helpers shared by the loss kernels (loss.hip: mkb_adversarial; ns_loss.hip: mkb_ns_loss): the fixed-order weight-sum
// tree and the hardware exp / log forms.  Fixed trees only: whoever sums with these gets the same bits run to run.
#pragma once
#include "common.h"
#include "model_math.h"

namespace mkb {

// (the first 256 lanes of the workgroup do the work: the same tree, hence the same bits, for 256- and 512-lane workgroups)
__device__ __forceinline__ float block_sum_256(float v, float *red) {
    v = wave_sum(v);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0 && wave < 4) red[wave] = v;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}

// the same sum with its first four strides' loads already made by the caller (v[z] = w[min(tid + 256 z, B - 1)], lanes < 256):
// the loss rows request them in front of their own loads
__device__ __forceinline__ float weight_sum_block_ahead(const float *__restrict__ w, int B, float *red, const float (&v)[4]) {
    float acc = 0.f;
    if (threadIdx.x < 256) {
#pragma unroll
        for (int z = 0; z < 4; ++z) acc += (int)threadIdx.x + 256 * z < B ? v[z] : 0.f;
        for (int i0 = threadIdx.x + 1024; i0 < B; i0 += 1024) {
            float u[4];
#pragma unroll
            for (int z = 0; z < 4; ++z) u[z] = w[min(i0 + 256 * z, B - 1)];
#pragma unroll
            for (int z = 0; z < 4; ++z) acc += i0 + 256 * z < B ? u[z] : 0.f;
        }
    }
    return block_sum_256(acc, red);
}

__device__ __forceinline__ float weight_sum_block(const float *__restrict__ w, int B, float *red) {
    // four strides' loads at a time (a loop with a run-time trip count is one round trip per iteration: every workgroup of the
    // loss launch walked 1024 weights in four of them); added in the order of the plain loop
    float acc = 0.f;
    if (threadIdx.x < 256)
        for (int i0 = threadIdx.x; i0 < B; i0 += 1024) {
            float v[4];
#pragma unroll
            for (int z = 0; z < 4; ++z) v[z] = w[min(i0 + 256 * z, B - 1)];
#pragma unroll
            for (int z = 0; z < 4; ++z) acc += i0 + 256 * z < B ? v[z] : 0.f;
        }
    return block_sum_256(acc, red);
}

// scal[0] = W by one 256-lane workgroup: the launch in front of a kernel whose workgroups are too many to re-reduce W each
// (ns_loss.hip, reg_rows.hip)
static __global__ __launch_bounds__(256) void weight_sum_kernel(const float *__restrict__ w, int B, float *__restrict__ scal) {
    __shared__ float red[4];
    const float acc = weight_sum_block(w, B, red);
    if (threadIdx.x == 0) scal[0] = acc;
}

// exp / log on the hardware transcendental unit (v_exp_f32 / v_log_f32, ~1 ulp of the base-2 function): the arguments
// here are scores of magnitude <= ~20, so exp's relative error stays ~1e-6 and log1p's absolute error ~1e-7 -- two
// orders below the 1e-4 / 1e-5 parity tolerances -- at a tenth of the instructions of the correctly rounded libm forms.
__device__ __forceinline__ float fast_exp(float x) { return __builtin_amdgcn_exp2f(x * 1.44269504088896341f); }
__device__ __forceinline__ float fast_log(float x) { return 0.69314718055994531f * __builtin_amdgcn_logf(x); }
__device__ __forceinline__ float fast_log_sigmoid(float z) {  // min(z,0) - log1p(exp(-|z|)), the form ATen uses
    return fminf(z, 0.f) - 0.69314718055994531f * __builtin_amdgcn_logf(1.f + fast_exp(-fabsf(z)));
}
__device__ __forceinline__ float fast_sigmoid(float z) { return __builtin_amdgcn_rcpf(1.f + fast_exp(-z)); }

}  // namespace mkb
