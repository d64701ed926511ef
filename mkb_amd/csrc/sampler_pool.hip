// Negatives from a candidate pool that somebody else made (include/mkb_hip.h, "pool samplers"): the per-row filter of a GIVEN
// pool of 2K entity ids, and the one device-side pool source that is not plain indexing, the alias-method draw.  No reference
// counterpart to match bit for bit (the uniform sampler of sampler.hip has one): membership is exact, the pool may repeat ids.
//
// mkb_pool_filter, one wave per batch row, 4 rows per 256-lane workgroup (1 when 2K > 1024):
//   the pool is staged once per workgroup in LDS; the row's known answers A_i are one contiguous range of the sorted key array of
//   its side (utils/true_keys.py), found by two binary searches as all_bce_kernel finds it; each lane then looks its pool entries
//   up in that range (a branch-free search whose step count is the same for every lane, four entries of a lane in flight
//   together), the kept positions are ballot-compacted in pool order into LDS, and the K slots, the position map and the
//   multiplicities are written from there -- the outputs of filter_rows_body (sampler_draw.h), with the same meaning.
//   Integer arithmetic only and one writer per output element: two runs give the same bytes.
// mkb_pool_draw_alias, one lane per pool entry: counter based like pool_draw_body's Philox draw, no state on the device.
#include "common.h"
#include "sampler_draw.h"

namespace mkb {

constexpr int kPoolFilterLanes = 256;
constexpr int kPoolFilterInFlight = 4;  // pool entries of one lane searched together

inline int pool_filter_rows_per_wg(int P) { return P <= 1024 ? kPoolFilterLanes / 64 : 1; }
inline size_t pool_filter_lds_bytes(int P, int rw) { return (size_t)P * sizeof(int64_t) + (size_t)rw * 2 * P * sizeof(int32_t); }

// smallest failing row, with its code, in status[0..1] (zeroed once by the caller, accumulated over calls): the pair is one
// 8-byte word (code in the low half = status[0]), so "unset" is told from "row 0" by the code, not by the row
__device__ __forceinline__ void record_empty_row(int32_t *status, int row) {
    unsigned long long *word = reinterpret_cast<unsigned long long *>(status);
    const unsigned long long mine = ((unsigned long long)(uint32_t)row << 32) | (uint32_t)(int32_t)MKB_ERR_EMPTY;
    unsigned long long cur = *word;
    for (;;) {
        if ((uint32_t)cur != 0u && (int32_t)(cur >> 32) <= row) return;
        const unsigned long long seen = atomicCAS(word, cur, mine);
        if (seen == cur) return;
        cur = seen;
    }
}

__global__ __launch_bounds__(kPoolFilterLanes) void pool_filter_kernel(
    const int64_t *__restrict__ sample, int B, int head_mode, int64_t N, int64_t R, const int64_t *__restrict__ pool, int K, int P,
    int rows_per_wg, const int64_t *__restrict__ keys, int64_t n_keys, int64_t *__restrict__ neg, int32_t *__restrict__ posmap,
    uint16_t *__restrict__ cnt, int64_t *__restrict__ touched, int32_t *__restrict__ status) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    int64_t *spool = reinterpret_cast<int64_t *>(lds_raw);  // [P]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wslot = wave < rows_per_wg ? wave : 0;  // idle waves alias slot 0 but never touch it
    int32_t *kept = reinterpret_cast<int32_t *>(spool + P) + (size_t)wslot * 2 * P;  // kept[rho] = position of the rho-th survivor
    int32_t *rank = kept + P;                                                         // rank[p] = rho or -1
    for (int e = threadIdx.x; e < P; e += kPoolFilterLanes) {
        const int64_t c = pool[e];
        spool[e] = c;
        if (touched && blockIdx.x == 0) touched[e] = c;  // id list of the rows a training step reads: pool | heads | tails
    }
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * rows_per_wg + wave;
    if (wave >= rows_per_wg || i >= B) return;  // (no workgroup barrier below: a wave owns its row and its LDS slot)
    const int64_t h = sample[3 * i], r = sample[3 * i + 1], t = sample[3 * i + 2];
    if (touched && lane == 0) { touched[P + i] = h; touched[P + B + i] = t; }
    const int64_t fixed = head_mode ? t : h, target = head_mode ? h : t;
    // A_i = keys[lo .. hi): the keys of query (fixed, r).  A fixed entity or relation outside its table has no known answer.
    int64_t lo = 0, m = 0, base = 0;
    if (keys && n_keys > 0 && fixed >= 0 && fixed < N && r >= 0 && r < R) {
        base = (fixed * R + r) * N;
        lo = lower_bound_dev(keys, n_keys, base);
        m = lower_bound_dev(keys, n_keys, base + N) - lo;
    }
    const int64_t *__restrict__ A = keys + lo;
    int nf = 0;
    for (int p0 = 0; p0 < P; p0 += 64 * kPoolFilterInFlight) {
        int64_t c[kPoolFilterInFlight], v[kPoolFilterInFlight];
        const int64_t *b[kPoolFilterInFlight];
#pragma unroll
        for (int u = 0; u < kPoolFilterInFlight; ++u) {
            const int p = p0 + u * 64 + lane;
            c[u] = p < P ? spool[p] : -1;
            v[u] = base + c[u];  // (an id outside [0, N) is never looked at as a member: see `in_table` below)
            b[u] = A;
        }
        // lower bound of v in A[0 .. m), branch free: every load is inside A[0 .. m) whatever v is
        for (int64_t len = m; len > 1;) {
            const int64_t half = len >> 1;
#pragma unroll
            for (int u = 0; u < kPoolFilterInFlight; ++u)
                if (b[u][half - 1] < v[u]) b[u] += half;
            len -= half;
        }
#pragma unroll
        for (int u = 0; u < kPoolFilterInFlight; ++u) {
            const int pb = p0 + u * 64;
            if (pb >= P) break;  // (uniform)
            const int p = pb + lane;
            const bool in_table = c[u] >= 0 && c[u] < N;
            const bool member = m > 0 && in_table && b[u][0] == v[u];
            const bool keep = p < P && !member && c[u] != target;
            const unsigned long long bal = __ballot(keep);
            const int rho = nf + __popcll(bal & ((1ull << lane) - 1ull));
            if (keep) kept[rho] = p;
            if (p < P) rank[p] = keep ? rho : -1;
            nf += __popcll(bal);
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    if (nf == 0) {
        if (lane == 0) record_empty_row(status, (int)i);
        for (int j = lane; j < K; j += 64) {
            neg[i * K + j] = 0;
            if (posmap) posmap[i * K + j] = 0;
        }
        if (cnt) for (int p = lane; p < P; p += 64) cnt[i * P + p] = 0;
        return;
    }
    for (int j = lane; j < K; j += 64) {  // cyclic fill: concat(f, f, ...)[:K]
        const int pp = kept[j % nf];
        neg[i * K + j] = spool[pp];
        if (posmap) posmap[i * K + j] = pp;
    }
    if (cnt) {  // multiplicity of pool position p among the K slots of this row
        for (int p = lane; p < P; p += 64) {
            const int rho = rank[p];
            cnt[i * P + p] = (rho >= 0 && rho < K) ? (uint16_t)((K - 1 - rho) / nf + 1) : (uint16_t)0;
        }
    }
}

__global__ __launch_bounds__(256) void pool_draw_alias_kernel(const int64_t *__restrict__ accept, const int32_t *__restrict__ alias,
                                                              uint32_t rng, int P, unsigned long long seed, unsigned long long draw,
                                                              int64_t *__restrict__ pool, uint32_t *__restrict__ words) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= P) return;
    uint32_t mask = rng;
    mask |= mask >> 1; mask |= mask >> 2; mask |= mask >> 4; mask |= mask >> 8; mask |= mask >> 16;
    rocrand_state_philox4x32_10 st;
    rocrand_init(seed, draw * (unsigned long long)P + (unsigned long long)p, 0ull, &st);
    uint32_t w = 0, v = 0;
    if (rng != 0) {  // the column: uniform on [0, rng] by masked rejection, as pool_draw_body draws a pool entry
        do { w = rocrand(&st); v = w & mask; } while (v > rng);
    }
    const uint32_t u = rocrand(&st);
    pool[p] = (unsigned long long)u < (unsigned long long)accept[v] ? (int64_t)v : (int64_t)alias[v];
    if (words) { words[2 * p] = w; words[2 * p + 1] = u; }
}

}  // namespace mkb

using namespace mkb;

extern "C" int mkb_pool_filter(const int64_t *sample, int64_t B, int mode, int64_t n_entity, int64_t n_relation, const int64_t *pool,
                               int64_t K, const int64_t *keys, int64_t n_keys, int64_t *neg, int32_t *pos, uint16_t *cnt,
                               int64_t *touched, int32_t *status, void *stream) {
    MKB_REQUIRE(sample && pool && neg && status, "null sample / pool / neg / status");
    MKB_REQUIRE(mode == MKB_MODE_HEAD || mode == MKB_MODE_TAIL, "the pool filter needs head-batch or tail-batch");
    MKB_REQUIRE(K >= 1 && K <= 1024, "size must be in [1, 1024], not %lld", (long long)K);
    MKB_REQUIRE(B >= 1 && B <= INT32_MAX, "bad B %lld", (long long)B);
    MKB_REQUIRE(n_entity >= 1 && n_entity < INT32_MAX + 1ll, "n_entity must be in [1, 2^31 - 1], not %lld", (long long)n_entity);
    MKB_REQUIRE(n_relation >= 1 && n_relation < INT32_MAX + 1ll, "n_relation must be in [1, 2^31 - 1], not %lld", (long long)n_relation);
    MKB_REQUIRE(n_keys >= 0 && (n_keys == 0 || keys), "n_keys %lld without keys", (long long)n_keys);
    MKB_REQUIRE(((uintptr_t)status & 7) == 0, "status must be 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const int P = (int)(2 * K), rw = pool_filter_rows_per_wg(P);
    ProfScope ps(MKB_PROF_SAMPLER, st);
    hipLaunchKernelGGL(pool_filter_kernel, dim3((unsigned)((B + rw - 1) / rw)), dim3(kPoolFilterLanes), pool_filter_lds_bytes(P, rw), st,
                       sample, (int)B, mode == MKB_MODE_HEAD ? 1 : 0, n_entity, n_relation, pool, (int)K, P, rw, n_keys ? keys : nullptr,
                       n_keys, neg, pos, cnt, touched, status);
    MKB_LAUNCH_CHECK();
    return MKB_OK;
}

extern "C" int mkb_pool_draw_alias(const int64_t *accept, const int32_t *alias, int64_t n_entity, int64_t K, uint64_t seed, uint64_t draw,
                                   int64_t *pool, uint32_t *words, void *stream) {
    MKB_REQUIRE(accept && alias && pool, "null accept / alias / pool");
    MKB_REQUIRE(K >= 1 && K <= 1024, "size must be in [1, 1024], not %lld", (long long)K);
    MKB_REQUIRE(n_entity >= 1 && n_entity < INT32_MAX + 1ll, "n_entity must be in [1, 2^31 - 1], not %lld", (long long)n_entity);
    hipStream_t st = (hipStream_t)stream;
    const int P = (int)(2 * K);
    ProfScope ps(MKB_PROF_SAMPLER, st);
    hipLaunchKernelGGL(pool_draw_alias_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, st, accept, alias, (uint32_t)(n_entity - 1), P,
                       (unsigned long long)seed, (unsigned long long)draw, pool, words);
    MKB_LAUNCH_CHECK();
    return MKB_OK;
}
