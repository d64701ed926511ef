// What the row losses share (loss.hip, ns_loss.hip, score_all.hip, reg_rows.hip, kl.hip; score_pool.hip embeds the finish): the
// protocol behind "one term per batch row, loss = c sum_i row_i / W" -- who reduces W = sum_i w_i, when one launch goes in front,
// where W and the row terms live in the scratch, how they become the loss (RowLoss, row_loss_weight_sum, row_loss_finish_*) -- the
// fixed-order trees under it and the hardware exp / log forms.  Fixed trees only: whoever sums with these gets the same bits run to
// run.
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

// scal[0] = W by one 256-lane workgroup: the launch RowLoss::open puts in front of a kernel whose workgroups are too many to
// re-reduce W each
static __global__ __launch_bounds__(256) void weight_sum_kernel(const float *__restrict__ w, int B, float *__restrict__ scal) {
    __shared__ float red[4];
    const float acc = weight_sum_block(w, B, red);
    if (threadIdx.x == 0) scal[0] = acc;
}

// W inside a row kernel: the caller's (scal), or reduced here by every workgroup alike (bit-identical in each), or B without weights
__device__ __forceinline__ float row_loss_weight_sum(const float *scal, const float *w, int B, float *red) {
    return scal ? scal[0] : (w ? weight_sum_block(w, B, red) : (float)B);
}
// ... and workgroup 0 publishes what it reduced in scal_out, for the finish
__device__ __forceinline__ float row_loss_weight_sum(const float *scal, float *scal_out, const float *w, int B, float *red) {
    const float W = row_loss_weight_sum(scal, w, B, red);
    if (!scal && blockIdx.x == 0 && threadIdx.x == 0) scal_out[0] = W;
    return W;
}
// ... with the first four strides of the weights (w is not null) loaded ahead by the caller: weight_sum_block_ahead
__device__ __forceinline__ float row_loss_weight_sum(const float *scal, float *scal_out, const float *w, int B, float *red,
                                                     const float (&v)[4]) {
    const float W = scal ? scal[0] : weight_sum_block_ahead(w, B, red, v);
    if (!scal && blockIdx.x == 0 && threadIdx.x == 0) scal_out[0] = W;
    return W;
}

// out[0] = c * sum_i rowpart[i] / W (scal null: W = 1) by ONE 256-lane workgroup, fixed order (strided partial sums, wave64
// butterfly, then the four wave totals left to right): bit-reproducible.  red: 4 floats of LDS.
__device__ __forceinline__ void row_loss_finish_block(const float *__restrict__ rowpart, int n, float c, const float *__restrict__ scal,
                                                      float *__restrict__ out, float *red) {
    float acc = 0.f;
    for (int i = threadIdx.x; i < n; i += 256) acc += rowpart[i];
    const float total = block_sum_256(acc, red);
    if (threadIdx.x == 0) out[0] = c * total / (scal ? scal[0] : 1.f);
}
static __global__ __launch_bounds__(256) void row_loss_finish_kernel(const float *__restrict__ rowpart, int n, float c,
                                                                     const float *__restrict__ scal, float *__restrict__ out) {
    __shared__ float red[4];
    row_loss_finish_block(rowpart, n, c, scal, out, red);
}

// Host side of the protocol.  scratch: [0] = W, [1 .. B] = the rows' terms.
struct RowLoss {
    // up to this many rows every workgroup of the row kernel re-reduces W itself (B / 256 loads per lane from L2); beyond, its
    // workgroups are too many for that and one weight_sum_kernel launch goes in front
    static constexpr int64_t kMaxRowsReducingW = 8192;

    const float *scal_in;  // the row kernel's `scal`: W on the device (the caller's, or the front launch's), or null = reduce it
    float *scal_out;       // where workgroup 0 of the row kernel publishes the W it reduced
    float *rowpart;        // [B] the rows' terms
    const float *scal;     // what the finish divides by

    // weight_sum: W of the whole (sharded) batch when the caller supplies it; weight may be null (W = B)
    static RowLoss open(const float *weight, const float *weight_sum, int64_t B, float *scratch, hipStream_t st) {
        RowLoss L{weight_sum, scratch, scratch + 1, weight_sum ? weight_sum : scratch};
        if (!weight_sum && weight && B > kMaxRowsReducingW) {
            hipLaunchKernelGGL(weight_sum_kernel, dim3(1), dim3(256), 0, st, weight, (int)B, scratch);
            L.scal_in = scratch;
        }
        return L;
    }
    void finish(int64_t B, float c, float *loss, hipStream_t st) const {
        hipLaunchKernelGGL(row_loss_finish_kernel, dim3(1), dim3(256), 0, st, rowpart, (int)B, c, scal, loss);
    }
};

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
