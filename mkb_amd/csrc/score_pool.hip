// Pooled scoring path: host driver, row kernels and the C-ABI entry points (mkb_pool_step / mkb_pool_score_fwd /
// mkb_pool_score_bwd).  The three tile kernels live in score_pool_kernels.h and are instantiated per model in
// score_pool_<model>.hip (parallel compilation); see the header for the design.
#include "score_pool_plan.h"
#include "query_side.h"
#include "gemm_mfma.h"
#include "loss_math.h"  // RowLoss, row_loss_finish_block

#include <stdlib.h>
#include <algorithm>

namespace mkb {

// ------------------------------------------------------------------------------------------------ row kernels
// One workgroup of 256 lanes per batch row.  What they know about a row's query -- operand rows, unit layout, build and chain --
// is query_side.h's; the query build itself (query_build_kernel, RowArgs) is that header's kernel, the very code the general
// path and the evaluation launch.

// sum of the slice partials of dQ for N elements of one row: the loads of four slices x N elements are requested together
// and added in slice order.  (A plain loop over a run-time slice count waits for every load before it issues the next: the
// ISA of row_bwd had 8 serial L2 round trips per lane and loop iteration there -- 32 per workgroup, most of the launch.)
template <int N>
__device__ __forceinline__ void dq_slices_sum(const float *__restrict__ dq, int64_t sstride, int nslices, const int (&k)[N], float (&out)[N]) {
#pragma unroll
    for (int e = 0; e < N; ++e) out[e] = 0.f;
    for (int s0 = 0; s0 < nslices; s0 += 4) {
        float v[4][N];
#pragma unroll
        for (int z = 0; z < 4; ++z) {
            const float *src = dq + (int64_t)min(s0 + z, nslices - 1) * sstride;
#pragma unroll
            for (int e = 0; e < N; ++e) v[z][e] = src[k[e]];
        }
#pragma unroll
        for (int z = 0; z < 4; ++z)
#pragma unroll
            for (int e = 0; e < N; ++e) out[e] += s0 + z < nslices ? v[z][e] : 0.f;
    }
}

// chain dQ[i] (sum of the slice partials) into the fixed operands' gradient rows (duplicate rows add: atomics)
template <int MODEL, bool HEAD>
__global__ __launch_bounds__(256) void query_bwd_kernel(RowArgs A) {
    const int64_t i = blockIdx.x;
    const QueryRow R = query_row<MODEL>(A, A.sample, i);
    const float *dq = A.Q + i * A.De;
    const int64_t sstride = (int64_t)A.B * A.De;
    float *g_e = A.g_ent + R.ent_id<HEAD>() * A.De;
    float *g_r = A.g_rel + R.r * A.Dr;
    for (int u = threadIdx.x; u < R.U; u += 256) {
        constexpr int N = ModelTraits<MODEL>::cplx_query ? 2 : 1;  // floats per unit
        Cplx de, dr;
        float dqn[N];
        if constexpr (N == 2) dq_slices_sum<2>(dq, sstride, A.nslices, {u, R.d + u}, dqn);
        else dq_slices_sum<1>(dq, sstride, A.nslices, {u}, dqn);
        query_unit_bwd<MODEL, HEAD>(R, u, dqn[0], dqn[N - 1], de, dr);  // (real models: dq1 is not read)
        query_grad_atomic<MODEL, HEAD>(g_e, g_r, R.d, u, de, dr);
    }
}

// ---- fused row kernels of the training step --------------------------------------------------------------
// One workgroup per batch row, lanes own units.  They replace four launches of the step (general forward and
// backward for the positive triple, query build, query backward) by two, read h / r / t rows once, and merge
// the positive- and negative-path contributions to the same table row before the (single) atomic per element.
struct RowStepArgs {
    const float *ent, *rel, *modulus;
    const int64_t *sample;
    float *Q;                 // [B, De] negative-path queries (out of row_fwd)
    const float *dQ;          // [nslices, B, De] partials (in of row_bwd)
    float *pos_score;         // [B] out of row_fwd
    const float *dpos;        // [B] d loss / d pos_score (in of row_bwd)
    float *g_ent, *g_rel, *g_modulus;
    int64_t De, Dr;
    int d, B, nslices;
    float kd, gamma;
    // row_bwd inside mkb_pool_step: its last workgroup also finishes the loss (row_loss_finish_block), or nullptr
    const float *loss_rowpart, *loss_scal;
    float *loss_out;
    // ... and extra workgroups behind the B row workgroups reduce the dx partials of the single-pass backward (blocks > 0)
    DxReduce dx;
    // ... or (MFMA path) add the split-K partials of the scattered product into the table gradient (kind 2: sc.M workgroups)
    GemmTail sc;
    // few relations (WN18RR: 11, YAGO3-10: 37): ~B / R rows of a batch add into the SAME gradient row, and same-line atomics
    // serialise in L2.  Row i then adds into copy (i % rel_copies) of a [copies, R, Dr] scratch that the row forward zeroed;
    // rel_fold_kernel adds the copies into g_rel behind the row backward.  rel_copies <= 1: straight into g_rel.
    float *rel_rep;
    int rel_copies, n_rel;
    // Exclusive rows.  occ[e] = how often entity e occurs among this batch's pool ids, heads and tails: zeroed for exactly
    // those entries by row_fwd, counted by the pooled forward (MFMA path: by the loss kernel), read by row_bwd.  An h / t
    // row that occurs once is written by
    // ONE workgroup of the row backward and by nobody else in that launch (the riders only write pool rows): it takes a
    // plain read-modify-write instead of one L2 atomic per element (the L2 atomic units retire ~1 element per clock and
    // channel: row_bwd was bound by them; 72 % of the heads and 57 % of the tails of an FB15k-237 batch occur once).
    int *occ;
    const int64_t *pool;
    int P;
    // GEMM route: depth[i] = one past the last pool position row i uses, written by row_fwd (see RowArgs::depth)
    const uint16_t *cnt;
    int *depth;
    int depth_P;
    // (Round 4 tried 16 bytes per lane with every load of a row issued before the first use -- 125 VGPRs, half the resident
    // waves, atomics at stride 16: row_bwd 29 -> 53 us at the headline shape.  The row kernels are bound by bytes and by
    // the L2 atomic units, not by the latency of their loads: 32 waves per CU hide that.  Removed.)
    // row_bwd: the gradient rows this step writes are known to be all-zero (the row-lazy optimizer's advance launch consumed
    // and cleared them): rows written by exactly one workgroup are STORED, not read-modified-written
    int grads_clear;
};

// positive score (mode None == tail-style formula against the true tail, pipeline.py:211) + Q for the negatives
template <int MODEL, bool HEAD>
__global__ __launch_bounds__(256) void row_fwd_kernel(RowStepArgs A) {
    __shared__ float red[4];
    const int64_t i = blockIdx.x;
    const QueryRow R = query_row<MODEL>(A, A.sample, i);
    float *q = A.Q + i * A.De;
    float acc = 0.f;
    if constexpr (ModelTraits<MODEL>::cplx_query) {
        for (int u = threadIdx.x; u < R.U; u += 256) {
            const Cplx ch = ent_unit(R.eh, R.d, u), ct = ent_unit(R.et, R.d, u);
            const Cplx cr = rel_unit<MODEL>(R.er, R.d, u);
            const Cplx qp = query_of<MODEL, false>(ch, cr, A.kd);
            const Cplx qn = HEAD ? query_of<MODEL, true>(ct, cr, A.kd) : qp;
            q[u] = qn.re;
            q[A.d + u] = qn.im;
            if constexpr (ModelTraits<MODEL>::cplx_pair) acc += pair_term_cmod(qp, ct);
            else acc += pair_term_real<MODEL, false>(qp.re, ct.re, A.kd) + pair_term_real<MODEL, false>(qp.im, ct.im, A.kd);
        }
    } else {
        for (int u = threadIdx.x; u < R.U; u += 256) {
            const float vh = R.eh[u], vr = R.er[u], vt = R.et[u];
            const float qp = query_of<MODEL, false>(vh, vr, A.kd);
            q[u] = HEAD ? query_of<MODEL, true>(vt, vr, A.kd) : qp;
            acc += pair_term_real<MODEL, false>(qp, vt, A.kd);
        }
    }
    acc = block_sum_4waves(acc, red);
    if (threadIdx.x == 0) A.pos_score[i] = finish_score<MODEL>(acc, A.gamma, MODEL == MKB_PROTATE ? A.modulus[0] : 0.f);
    if (A.depth) row_depth_256(A.cnt, A.depth_P, i, A.depth);
    // housekeeping for the later kernels of the step, behind the row's own work (fire-and-forget stores)
    if (A.occ && threadIdx.x == 64) {  // (counted by the pooled forward / the loss kernel, read by the row backward)
        A.occ[R.h] = 0; A.occ[R.t] = 0;
        for (int64_t p = i; p < A.P; p += A.B) A.occ[A.pool[p]] = 0;
    }
    if (A.rel_copies > 1)  // the row backward's relation-gradient copies start from zero
        for (int64_t e = i * 256 + threadIdx.x; e < (int64_t)A.rel_copies * A.n_rel * A.Dr; e += (int64_t)A.B * 256) A.rel_rep[e] = 0.f;
}

// backward of the positive pair + chain of both query gradients into the rows of h, r, t
template <int MODEL, bool HEAD>
__global__ __launch_bounds__(256) void row_bwd_kernel(RowStepArgs A) {
    __shared__ float red[4];
    // rider: dx partial reduction of the pooled backward (one launch fewer per step).  Its workgroups come FIRST: they are
    // few and heavy (8 partial rows each); dispatched behind the 1024 row workgroups they formed a 30 us tail.
    if ((int)blockIdx.x < A.dx.blocks) {
        pool_dx_reduce_block(A.dx, (int)blockIdx.x);
        return;
    }
    const int sc_blocks = A.sc.kind == 2 ? A.sc.M : 0;
    if ((int)blockIdx.x < A.dx.blocks + sc_blocks) {
        __shared__ int s_red[16];
        splitk_scatter_block(A.sc.part, A.sc.out, A.sc.c_idx, A.sc.M, A.sc.N, A.sc.ldc, A.sc.nz, (int)blockIdx.x - A.dx.blocks,
                             A.sc.depth, A.sc.n_depth, s_red);
        return;
    }
    const int64_t i = (int64_t)blockIdx.x - A.dx.blocks - sc_blocks;
    const QueryRow R = query_row<MODEL>(A, A.sample, i);
    float *g_h = A.g_ent + R.h * A.De, *g_t = A.g_ent + R.t * A.De;
    float *g_r = A.rel_copies > 1 ? A.rel_rep + ((int64_t)(i % A.rel_copies) * A.n_rel + R.r) * A.Dr : A.g_rel + R.r * A.Dr;
    const float *dq = A.dQ + i * A.De;
    const int64_t sstride = (int64_t)A.B * A.De;
    const float gp = A.dpos[i];
    const bool own_h = A.occ && A.occ[R.h] == 1, own_t = A.occ && A.occ[R.t] == 1;  // workgroup-uniform
    // rows one workgroup alone writes: a plain store when the row is known to be all-zero (grads_clear), else read-modify-
    // write; shared rows: one fp32 atomic per element
    const bool st_h = own_h && A.grads_clear, st_t = own_t && A.grads_clear;  // workgroup-uniform
    auto add_h = [&](int k, float v) { if (st_h) g_h[k] = v; else if (own_h) g_h[k] += v; else atomicAdd(g_h + k, v); };
    auto add_t = [&](int k, float v) { if (st_t) g_t[k] = v; else if (own_t) g_t[k] += v; else atomicAdd(g_t + k, v); };
    const float modulus = (MODEL == MKB_PROTATE) ? A.modulus[0] : 0.f;
    float extra = 0.f;
    if constexpr (ModelTraits<MODEL>::cplx_query) {
        for (int u = threadIdx.x; u < R.U; u += 256) {
            const Cplx ch = ent_unit(R.eh, R.d, u), ct = ent_unit(R.et, R.d, u);
            const Cplx cr = rel_unit<MODEL>(R.er, R.d, u);
            // positive pair: q = h (x) rot, candidate = t
            const Cplx qp = query_of<MODEL, false>(ch, cr, A.kd);
            Cplx dqp, dxp;
            if constexpr (ModelTraits<MODEL>::cplx_pair) {
                pair_bwd_cmod(qp, ct, gp, dqp, dxp);
            } else {
                float e0 = 0.f;
                pair_bwd_real<MODEL, false>(qp.re, ct.re, gp, A.kd, modulus, dqp.re, dxp.re, e0);
                pair_bwd_real<MODEL, false>(qp.im, ct.im, gp, A.kd, modulus, dqp.im, dxp.im, e0);
            }
            Cplx dh, dr, dt = dxp, de, dr2;
            query_chain<MODEL, false>(ch, cr, dqp, A.kd, dh, dr);
            // negative path: q = conj(rot) (x) t (head-batch) or h (x) rot (tail-batch)
            float dqs[2];
            dq_slices_sum<2>(dq, sstride, A.nslices, {u, A.d + u}, dqs);
            const Cplx dqn{dqs[0], dqs[1]};
            query_chain<MODEL, HEAD>(HEAD ? ct : ch, cr, dqn, A.kd, de, dr2);
            if constexpr (HEAD) { dt.re += de.re; dt.im += de.im; } else { dh.re += de.re; dh.im += de.im; }
            dr.re += dr2.re; dr.im += dr2.im;
            add_h(u, dh.re); add_h(A.d + u, dh.im);
            add_t(u, dt.re); add_t(A.d + u, dt.im);
            atomicAdd(g_r + u, dr.re);
            if constexpr (MODEL == MKB_COMPLEX) atomicAdd(g_r + A.d + u, dr.im);
        }
    } else {
        for (int u = threadIdx.x; u < R.U; u += 256) {
            const float vh = R.eh[u], vr = R.er[u], vt = R.et[u];
            const float qp = query_of<MODEL, false>(vh, vr, A.kd);
            float dqp, dxp, e0 = 0.f;
            pair_bwd_real<MODEL, false>(qp, vt, gp, A.kd, modulus, dqp, dxp, e0);
            extra += gp * e0;
            float dh, dr, dt = dxp;
            query_chain<MODEL, false>(vh, vr, dqp, A.kd, dh, dr);
            float de, dr2, dqs[1];
            dq_slices_sum<1>(dq, sstride, A.nslices, {u}, dqs);
            query_chain<MODEL, HEAD>(HEAD ? vt : vh, vr, dqs[0], A.kd, de, dr2);
            if constexpr (HEAD) dt += de; else dh += de;
            dr += dr2;
            add_h(u, dh);
            atomicAdd(g_r + u, dr);
            add_t(u, dt);
        }
    }
    if constexpr (MODEL == MKB_PROTATE) {  // d score / d modulus = - sum_k |sin z| for the positive pair
        extra = block_sum_4waves(extra, red);
        if (threadIdx.x == 0) atomicAdd(A.g_modulus, -extra);
    }
    if (A.loss_out && i == A.B - 1) {  // the per-row loss terms were written by an earlier kernel
        __builtin_assume(A.loss_scal != nullptr);  // (set together with loss_out: the finish has no W = 1 case to select here)
        row_loss_finish_block(A.loss_rowpart, A.B, -0.5f, A.loss_scal, A.loss_out, red);
    }
}

// g_rel[e] += sum_c rep[c][e]   (fixed order; rep was zeroed by this step's loss kernel)
__global__ __launch_bounds__(256) void rel_fold_kernel(const float *__restrict__ rep, float *__restrict__ g_rel, int copies, int64_t n) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    // eight copies' loads at a time (a loop with a run-time trip count waits for every load before it issues the next:
    // 23 copies were 23 round trips -- 7 us for half a megabyte); added up in copy order
    float s = 0.f;
    const float old = g_rel[e];
    for (int c0 = 0; c0 < copies; c0 += 8) {
        float v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = rep[(int64_t)min(c0 + k, copies - 1) * n + e];
#pragma unroll
        for (int k = 0; k < 8; ++k) s += c0 + k < copies ? v[k] : 0.f;
    }
    g_rel[e] = old + s;
}

__global__ __launch_bounds__(256) void masked_copy_kernel(const float *__restrict__ src, const uint16_t *__restrict__ cnt,
                                                          float *__restrict__ dst, int64_t n, int64_t n_pad, int64_t P, SeedLayout SL) {
    // n = B * P entries of the batch; [n, n_pad): the rows that pad the last tile of 8 in the blocked layout, written as 0
    // (the dense pass of the single-pass backward reads a tile's 8 seeds without looking at B)
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) dst[seed_index(SL, i / P, i % P, P)] = cnt[i] ? src[i] : 0.f;
    else if (i < n_pad) dst[seed_index(SL, i / P, i % P, P)] = 0.f;
}

// ------------------------------------------------------------------------------------------------ host side
struct Workspace {
    float *Q, *dQ, *G, *dpos, *scratch, *gemm_part, *dXp;
    unsigned long long *xused;
    float *rel_rep;
    int *occ;
    int *depth;  // [B] used pool depth per row (GEMM route)
    float *tile_part;
    size_t bytes;
};

static size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// read once per ABI call (the tests switch them within one process)
static PoolSwitches switches_from_env() {
    const char *m = getenv("MKB_POOL_NO_MFMA"), *d = getenv("MKB_POOL_DENSE");
    return PoolSwitches{m && m[0] == '1', !d ? PoolSwitches::kDenseDefault : (d[0] == '1' ? PoolSwitches::kDenseOn : PoolSwitches::kDenseOff),
                        gemm_switches_from_env()};
}

// Callers cache a workspace per table shape while the per-call switches change the layout: mkb_pool_step_workspace_bytes
// reports the largest layout over the switches' settings.
static Workspace carve(void *ws, int64_t B, int64_t P, int64_t De, const PoolPlan &L) {
    Workspace w;
    unsigned char *p = (unsigned char *)ws;
    size_t off = 0;
    auto take = [&](size_t n) { void *r = p ? p + off : nullptr; off += align256(n); return (float *)r; };
    const bool sp = L.single_pass();
    w.Q = take((size_t)B * De * 4);
    w.dQ = take((size_t)(L.matrix() ? kMfmaDqSlices : L.dq_parts) * B * De * 4);  // (Matrix: the cap its dQ plan was given)
    // gradient seeds: plain [B, P], or the tile-blocked layout of the single-pass backward
    const size_t g_plain = (size_t)B * P, g_blocked = sp ? L.single.seed_elems(B) : 0;
    w.G = take((g_plain > g_blocked ? g_plain : g_blocked) * 4);
    w.dpos = take((size_t)B * 4);
    w.scratch = take((size_t)(B + 1) * 4);
    w.gemm_part = take(L.matrix() ? L.gemm_part * 4 : 0);  // split-K partials of the matrix route, sized by its plans
    w.dXp = take(sp ? L.single.dxp_elems() * 4 : 0);
    w.xused = (unsigned long long *)take(sp ? L.single.xused_words() * 8 : 0);
    w.rel_rep = take(L.rel_copies > 1 ? (size_t)L.rel_copies * L.rel_elems * 4 : 0);
    w.occ = (int *)take((size_t)L.n_entity * 4);
    w.depth = (int *)take(L.matrix() ? (size_t)B * 4 : 0);
    w.tile_part = take(L.fwd == FwdRoute::Tile ? (size_t)L.tile.ks * B * L.tile.kd * 4 : 0);  // dim-split partial scores of the dense prefix
    w.bytes = off;
    return w;
}

#ifdef MKB_TRACE_WG
static unsigned long long *g_trace = nullptr;
static int g_trace_kind = 2;
extern "C" void mkb_debug_set_trace(void *p, int kind) { g_trace = (unsigned long long *)p; g_trace_kind = kind; }
#endif

// every PoolArgs field that follows from the tables, the workspace and the plan (bwd: of the plan's backward route)
static PoolArgs make_args(const mkb_tables_t *tb, const int64_t *pool, const uint16_t *cnt, int64_t B, int64_t P,
                          const Workspace &w, const PoolPlan &L, bool bwd) {
    PoolArgs A{};
    A.ent = tb->ent; A.Q = w.Q; A.pool = pool; A.cnt = cnt; A.G = w.G; A.dQ = w.dQ;
    A.B = (int)B; A.P = (int)P; A.d = tb->hidden_dim; A.De = tb->entity_dim; A.kd = tb->phase_div;
    A.modulus = tb->modulus;
    const bool g = tb->model == MKB_TRANSE || tb->model == MKB_ROTATE || tb->model == MKB_PROTATE;
    A.c0 = g ? tb->gamma : 0.f;
    A.c1 = g ? -1.f : 1.f;
    if (bwd) switch (L.bwd) {
        case BwdRoute::SinglePass:
            A.q_slices = L.single.blocks; A.dim_slices = L.single.dim_slices; A.pb_halves = L.single.halves;
            A.tiles_per_wave = L.single.tiles_per_wave; A.dense_lanes = L.single.dense_lanes;
            A.lds_ids_off = L.single.lds_ids_off();
            A.dXp = w.dXp; A.xused = w.xused; A.g_blocked = 1;
            break;
        case BwdRoute::Wave: A.q_slices = L.wave.slices; break;
        case BwdRoute::TwoPass: A.q_slices = L.two.q_slices; A.x_slices = L.two.x_slices; break;
        case BwdRoute::Matrix: break;
    }
#ifdef MKB_TRACE_WG
    A.trace = g_trace; A.trace_kind = g_trace_kind;
#endif
    return A;
}

static int launch_tiles(const mkb_tables_t *tb, bool head, int which, const PoolPlan &L, const PoolArgs &A, hipStream_t st) {
    return dispatch_model_side(tb->model, head, [&](auto m, auto h) { return pool_launch<m(), h()>(which, L, A, st); });
}

// The row kernels for the tables' model and the call's side: one workgroup of 256 lanes per batch row
template <class Args>
static int launch_rows(void (*kernel)(Args), unsigned blocks, const Args &ra, hipStream_t st) {
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(256), 0, st, ra);
    MKB_LAUNCH_CHECK();
    return MKB_OK;
}
static int launch_query_build(const mkb_tables_t *tb, bool head, const RowArgs &ra, hipStream_t st) {
    return dispatch_model_side(tb->model, head, [&](auto m, auto h) { return launch_rows(query_build_kernel<m(), h()>, (unsigned)ra.B, ra, st); });
}
static int launch_query_bwd(const mkb_tables_t *tb, bool head, const RowArgs &ra, hipStream_t st) {
    return dispatch_model_side(tb->model, head, [&](auto m, auto h) { return launch_rows(query_bwd_kernel<m(), h()>, (unsigned)ra.B, ra, st); });
}
static int launch_row_fwd(const mkb_tables_t *tb, bool head, const RowStepArgs &ra, hipStream_t st) {
    return dispatch_model_side(tb->model, head, [&](auto m, auto h) { return launch_rows(row_fwd_kernel<m(), h()>, (unsigned)ra.B, ra, st); });
}
static int launch_row_bwd(const mkb_tables_t *tb, bool head, const RowStepArgs &ra, hipStream_t st) {
    const unsigned blocks = (unsigned)(ra.B + ra.dx.blocks + (ra.sc.kind == 2 ? ra.sc.M : 0));  // (the riders' workgroups come first)
    return dispatch_model_side(tb->model, head, [&](auto m, auto h) { return launch_rows(row_bwd_kernel<m(), h()>, blocks, ra, st); });
}

// Q = the rows' queries; matrix route: + the used pool depth per row (GEMM cuts)
static int build_queries(const mkb_tables_t *tb, bool head, const int64_t *sample, const uint16_t *cnt, int64_t B, int64_t P,
                         const Workspace &w, const PoolPlan &L, hipStream_t st) {
    RowArgs ra{tb->ent, tb->rel, sample, w.Q, nullptr, nullptr, tb->entity_dim, tb->relation_dim, tb->hidden_dim, (int)B, 1,
               tb->phase_div};
    if (L.matrix()) { ra.cnt = cnt; ra.depth = w.depth; ra.P = (int)P; }
    return launch_query_build(tb, head, ra, st);
}

static int pooled_fwd(const mkb_tables_t *tb, bool head, const int64_t *sample, const int64_t *pool, const uint16_t *cnt,
                      int64_t B, int64_t P, float *S, const Workspace &w, const PoolPlan &L, hipStream_t st,
                      GemmTail *s_tail = nullptr, int *occ = nullptr) {
    if (s_tail) s_tail->kind = 0;
    ProfScope ps(MKB_PROF_POOL_FWD, st);
    if (L.fwd == FwdRoute::Matrix) {  // S = Q . ent[pool]^T on the matrix cores, over the pool positions the row tile uses (cnt masks later)
        GemmArgs g = gemm_args(L.gemm);
        g.A = w.Q; g.B = tb->ent; g.b_idx = pool; g.C = S; g.c0 = 0.f; g.c1 = 1.f;
        g.depth = w.depth; g.depth_mode = 1; g.n_depth = (int)B;
        return launch_gemm<true, true, GEMM_STORE_AFFINE>(L.gemm, g, st, w.gemm_part, s_tail);
    }
    PoolArgs A = make_args(tb, pool, cnt, B, P, w, L, /*bwd=*/false);  // (the kernel also zero-fills the entries no row uses)
    A.S = S;
    if (occ) { A.occ = occ; A.occ_sample = sample; }
    if (L.fwd == FwdRoute::Tile) {  // (s_tail: the loss rows of mkb_pool_step add the prefix's partial sums up; otherwise S is finished here)
        A.tile_part = w.tile_part;
        A.tile_tail = s_tail;
    }
    return launch_tiles(tb, head, kPoolFwd, L, A, st);
}

// the two products of the matrix route, as the plan has them: one launch or two
static int matrix_bwd(const mkb_tables_t *tb, const mkb_grads_t *gr, const int64_t *pool, int64_t B, const Workspace &w,
                      const BwdMatrix &M, hipStream_t st, GemmTail *x_tail) {
    // dQ [B, De] = G [B, P] . ent[pool]   (w.depth was written by this call's row_fwd / query_build)
    GemmArgs gq = gemm_args(M.dq);
    gq.A = w.G; gq.B = tb->ent; gq.b_idx = pool; gq.C = w.dQ;
    gq.depth = w.depth; gq.depth_mode = 2; gq.n_depth = (int)B;  // (G is exactly 0 beyond a row's depth)
    // g_ent[pool[p]] += (G^T [P, B] . Q [B, De])[p]
    GemmArgs gx = gemm_args(M.dx);
    gx.A = w.G; gx.B = w.Q; gx.C = gr->g_ent; gx.c_idx = pool;
    gx.depth = w.depth; gx.depth_mode = 3; gx.n_depth = (int)B;
    if (M.pair) {  // (profiled as the POOL_BWD_Q class)
        ProfScope ps(MKB_PROF_POOL_BWD_Q, st);
        return launch_gemm_bwd_pair(M.dq, gq, M.dx, gx, w.gemm_part, x_tail, st);
    }
    {
        ProfScope ps(MKB_PROF_POOL_BWD_Q, st);
        if (int rc = launch_gemm<true, false, GEMM_STORE>(M.dq, gq, st, w.gemm_part)) return rc;
    }
    ProfScope ps(MKB_PROF_POOL_BWD_X, st);
    return launch_gemm<false, false, GEMM_ATOMIC_ROWS>(M.dx, gx, st, w.gemm_part, x_tail);
}

// leaves L.dq_parts [B, De] partial products in the dQ buffer (the consumer -- row / query backward -- adds them up)
static int pooled_bwd(const mkb_tables_t *tb, bool head, const mkb_grads_t *gr, const int64_t *pool, const uint16_t *cnt, int64_t B,
                      int64_t P, const Workspace &w, const PoolPlan &L, hipStream_t st, DxReduce *dx_out, GemmTail *x_tail) {
    if (x_tail) x_tail->kind = 0;
    if (L.matrix()) return matrix_bwd(tb, gr, pool, B, w, L.products, st, x_tail);
    PoolArgs A = make_args(tb, pool, cnt, B, P, w, L, /*bwd=*/true);
    A.g_modulus = gr->g_modulus;
    A.g_ent = gr->g_ent;
    A.dx_reduce_out = dx_out;
    ProfScope ps(MKB_PROF_POOL_BWD_Q, st);  // (all three tile routes are profiled as the POOL_BWD_Q class)
    return launch_tiles(tb, head, kPoolBwd, L, A, st);
}

static int check_pool_call(const mkb_tables_t *tb, const int64_t *sample, const int64_t *pool, const uint16_t *cnt, int64_t B,
                           int64_t K, int mode, const void *ws, PoolFolds folds, PoolPlan &L) {
    if (int rc = validate_tables(tb)) return rc;
    MKB_REQUIRE(sample && pool && cnt && ws, "null pointer");
    MKB_REQUIRE(B > 0 && K > 0 && B <= INT32_MAX, "bad B / K");
    MKB_REQUIRE(tb->n_entity <= INT32_MAX, "n_entity too large");
    MKB_REQUIRE(mode == MKB_MODE_HEAD || mode == MKB_MODE_TAIL, "the pooled path needs head-batch or tail-batch");
    MKB_REQUIRE((((uintptr_t)ws) & 255) == 0, "workspace must be 256-byte aligned");
    if (2 * K > kMaxP || !plan_pool(tb, B, 2 * K, switches_from_env(), folds, L))
        return set_error(MKB_ERR_UNSUPPORTED, "shape not covered by the pooled kernels (size <= 1024, rows <= 4096 units, "
                                              "even dims above 256 units); use the general path");
    return MKB_OK;
}

}  // namespace mkb

using namespace mkb;

extern "C" int mkb_pool_supported(const mkb_tables_t *tb, int64_t B, int64_t K) {
    PoolPlan L;
    return tb && B > 0 && K > 0 && 2 * K <= kMaxP && tb->n_entity <= INT32_MAX && plan_pool(tb, B, 2 * K, switches_from_env(), PoolFolds{}, L);
}

extern "C" int64_t mkb_pool_step_workspace_bytes(const mkb_tables_t *tb, int64_t B, int64_t K) {
    if (!tb || B <= 0 || K <= 0) return 0;
    PoolPlan L;
    if (!plan_pool(tb, B, 2 * K, switches_from_env(), PoolFolds{}, L)) return 0;  // (the shape must be supported as the environment stands)
    int64_t best = 0;
    // (the matrix route's layout is the same under every setting of the three GEMM switches and whatever the call folds: its
    // buffers are sized by the bounds of its plans, PoolPlan::gemm_part and kMfmaDqSlices)
    for (bool no_mfma : {false, true})
        for (PoolSwitches::Dense dense : {PoolSwitches::kDenseOff, PoolSwitches::kDenseOn})
            if (plan_pool(tb, B, 2 * K, PoolSwitches{no_mfma, dense, GemmSwitches{}}, PoolFolds{}, L))
                best = std::max(best, (int64_t)carve(nullptr, B, 2 * K, tb->entity_dim, L).bytes);
    return best;
}

extern "C" int mkb_pool_score_fwd(const mkb_tables_t *tb, const int64_t *sample, const int64_t *pool, const uint16_t *cnt,
                                  int64_t B, int64_t K, int mode, float *pool_score, void *ws, void *stream) {
    PoolPlan L;
    if (int rc = check_pool_call(tb, sample, pool, cnt, B, K, mode, ws, PoolFolds{}, L)) return rc;
    MKB_REQUIRE(pool_score != nullptr, "pool_score is null");
    const Workspace w = carve(ws, B, 2 * K, tb->entity_dim, L);
    hipStream_t st = (hipStream_t)stream;
    if (int rc = build_queries(tb, mode_is_head(mode), sample, cnt, B, 2 * K, w, L, st)) return rc;
    return pooled_fwd(tb, mode_is_head(mode), sample, pool, cnt, B, 2 * K, pool_score, w, L, st);
}

extern "C" int mkb_pool_score_bwd(const mkb_tables_t *tb, const mkb_grads_t *gr, const int64_t *sample, const int64_t *pool,
                                  const uint16_t *cnt, int64_t B, int64_t K, int mode, const float *dpool_score, void *ws,
                                  void *stream) {
    PoolPlan L;
    if (int rc = check_pool_call(tb, sample, pool, cnt, B, K, mode, ws, PoolFolds{}, L)) return rc;
    MKB_REQUIRE(gr && gr->g_ent && gr->g_rel && dpool_score, "null pointer");
    MKB_REQUIRE(tb->model != MKB_PROTATE || gr->g_modulus, "pRotatE needs g_modulus");
    const int64_t P = 2 * K;
    const Workspace w = carve(ws, B, P, tb->entity_dim, L);
    hipStream_t st = (hipStream_t)stream;
    const bool head = mode_is_head(mode);
    // rebuild the queries (the forward's copy may have been overwritten by another call sharing the workspace)
    if (int rc = build_queries(tb, head, sample, cnt, B, P, w, L, st)) return rc;
    // G = caller's gradient with the entries no row uses forced to 0 (the single-pass backward reads the mask off G)
    const int64_t n_pad = (L.single_pass() ? Bwd1Layout::padded_rows(B) : B) * P;
    hipLaunchKernelGGL(masked_copy_kernel, dim3((unsigned)((n_pad + 255) / 256)), dim3(256), 0, st, dpool_score, cnt, w.G,
                       B * P, n_pad, P, L.seeds());
    MKB_LAUNCH_CHECK();
    if (int rc = pooled_bwd(tb, head, gr, pool, cnt, B, P, w, L, st, nullptr, nullptr)) return rc;
    // chain dQ into the fixed operands' gradient rows
    RowArgs ra{tb->ent, tb->rel, sample, w.dQ, gr->g_ent, gr->g_rel, tb->entity_dim, tb->relation_dim, tb->hidden_dim,
               (int)B, L.dq_parts, tb->phase_div};
    return launch_query_bwd(tb, head, ra, st);
}

// The two halves of mkb_pool_step.  Between them the caller may combine the scores of several devices that each
// hold a slice of the embedding DIMENSIONS (mkb_amd.parallel.DimSharded*): scores are sums over dims, so the halves'
// only coupling is pos_score / pool_score.
// s_tail (mkb_pool_step only): the MFMA forward may leave the scores as split-K partials for the loss rows to reduce
static int pool_step_fwd(const mkb_tables_t *tb, const int64_t *sample, const int64_t *pool, const uint16_t *cnt, int64_t B,
                         int64_t K, int mode, float *pos_score, float *pool_score, void *ws, void *stream, GemmTail *s_tail) {
    PoolPlan L;
    if (s_tail && 2 * K > 64 * 16) s_tail = nullptr;  // (the loss rows reduce the scores of pools of <= 1024 positions)
    if (int rc = check_pool_call(tb, sample, pool, cnt, B, K, mode, ws, PoolFolds{s_tail != nullptr, true}, L)) return rc;
    MKB_REQUIRE(pos_score && pool_score, "null pointer");
    const int64_t P = 2 * K;
    const Workspace w = carve(ws, B, P, tb->entity_dim, L);
    hipStream_t st = (hipStream_t)stream;
    const bool head = mode_is_head(mode);
    RowStepArgs ra{tb->ent, tb->rel, tb->modulus, sample, w.Q, w.dQ, pos_score, w.dpos, nullptr, nullptr, nullptr,
                   tb->entity_dim, tb->relation_dim, tb->hidden_dim, (int)B, L.dq_parts, tb->phase_div, tb->gamma};
    ra.occ = w.occ; ra.pool = pool; ra.P = (int)P;
    if (L.rel_copies > 1) { ra.rel_rep = w.rel_rep; ra.rel_copies = L.rel_copies; ra.n_rel = (int)tb->n_relation; }
    if (L.matrix()) { ra.cnt = cnt; ra.depth = w.depth; ra.depth_P = (int)P; }  // used pool depth per row (GEMM cuts)
    // positive pass (mode None: tail-style formula against the true tail, pipeline.py:211) + negative-path queries
    {
        ProfScope ps(MKB_PROF_GENERAL_FWD, st);
        if (int rc = launch_row_fwd(tb, head, ra, st)) return rc;
    }
    // negative pass over the shared pool (pipeline.py:230-232)
    return pooled_fwd(tb, head, sample, pool, cnt, B, P, pool_score, w, L, st, s_tail, ra.occ);
}

// s_tail: scores still in split-K partials (from pool_step_fwd); fold: the scattered product's tail rides the row backward
static int pool_step_bwd(const mkb_tables_t *tb, const mkb_grads_t *gr, const int64_t *sample, const float *weight,
                         const int64_t *pool, const uint16_t *cnt, int64_t B, int64_t K, int mode, float alpha,
                         const float *weight_sum, const float *pos_score, float *pool_score, float *loss, void *ws,
                         void *stream, const GemmTail *s_tail) {
    PoolPlan L;
    if (int rc = check_pool_call(tb, sample, pool, cnt, B, K, mode, ws, PoolFolds{s_tail != nullptr, true}, L)) return rc;
    MKB_REQUIRE(gr && gr->g_ent && gr->g_rel && weight && pos_score && pool_score && loss, "null pointer");
    MKB_REQUIRE(tb->model != MKB_PROTATE || gr->g_modulus, "pRotatE needs g_modulus");
    const int64_t P = 2 * K;
    const Workspace w = carve(ws, B, P, tb->entity_dim, L);
    hipStream_t st = (hipStream_t)stream;
    const bool head = mode_is_head(mode);
    RowStepArgs ra{tb->ent, tb->rel, tb->modulus, sample, w.Q, w.dQ, nullptr, w.dpos, gr->g_ent, gr->g_rel, gr->g_modulus,
                   tb->entity_dim, tb->relation_dim, tb->hidden_dim, (int)B, L.dq_parts, tb->phase_div, tb->gamma};
    // Adversarial forward + gradient seeds (pipeline.py:234 and the head of :236)
    ra.occ = w.occ; ra.pool = pool; ra.P = (int)P;
    if (L.rel_copies > 1) {  // (zeroed by the row forward kernel of this step)
        ra.rel_rep = w.rel_rep; ra.rel_copies = L.rel_copies; ra.n_rel = (int)tb->n_relation;
    }
    // (the occurrence counts: the VALU forward kernel counted them; the MFMA path has no such kernel, the loss rows do it)
    RowLoss rl;
    if (int rc = adversarial_launch(pos_score, pool_score, weight, cnt, B, P, alpha, weight_sum, loss, w.dpos, w.G, w.scratch, st,
                                    &rl, L.seeds(), s_tail, L.matrix() ? ra.occ : nullptr, sample, pool)) return rc;
    ra.loss_rowpart = rl.rowpart;
    ra.loss_scal = rl.scal;
    ra.loss_out = loss;
    // backward (pipeline.py:236): pooled negatives, then the positive pair and both query chains in one row kernel
    if (int rc = pooled_bwd(tb, head, gr, pool, cnt, B, P, w, L, st, L.single_pass() ? &ra.dx : nullptr, &ra.sc)) return rc;
    ra.dx.occ = ra.occ;  // (the dx reduction riding this launch writes pool rows: exclusive ones without atomics)
    ra.grads_clear = gr->rows_clear ? 1 : 0;
    ra.dx.clear = ra.grads_clear;
    ProfScope ps(MKB_PROF_GENERAL_BWD, st);
    if (int rc = launch_row_bwd(tb, head, ra, st)) return rc;
    if (ra.rel_rep) {
        hipLaunchKernelGGL(rel_fold_kernel, dim3((unsigned)((L.rel_elems + 255) / 256)), dim3(256), 0, st, ra.rel_rep, gr->g_rel,
                           L.rel_copies, L.rel_elems);
        MKB_LAUNCH_CHECK();
    }
    return MKB_OK;
}

extern "C" int mkb_pool_step_fwd(const mkb_tables_t *tb, const int64_t *sample, const int64_t *pool, const uint16_t *cnt,
                                 int64_t B, int64_t K, int mode, float *pos_score, float *pool_score, void *ws,
                                 void *stream) {
    return pool_step_fwd(tb, sample, pool, cnt, B, K, mode, pos_score, pool_score, ws, stream, nullptr);
}

extern "C" int mkb_pool_step_bwd(const mkb_tables_t *tb, const mkb_grads_t *gr, const int64_t *sample, const float *weight,
                                 const int64_t *pool, const uint16_t *cnt, int64_t B, int64_t K, int mode, float alpha,
                                 const float *weight_sum, const float *pos_score, const float *pool_score, float *loss,
                                 void *ws, void *stream) {
    return pool_step_bwd(tb, gr, sample, weight, pool, cnt, B, K, mode, alpha, weight_sum, pos_score,
                         const_cast<float *>(pool_score), loss, ws, stream, nullptr);
}

extern "C" int mkb_pool_step(const mkb_tables_t *tb, const mkb_grads_t *gr, const int64_t *sample, const float *weight,
                             const int64_t *pool, const uint16_t *cnt, int64_t B, int64_t K, int mode, float alpha,
                             const float *weight_sum, float *pos_score, float *pool_score, float *loss, void *ws,
                             void *stream) {
    // one call: the split-K tails of the MFMA products fold into the launches that follow them
    GemmTail s_tail{};
    if (int rc = pool_step_fwd(tb, sample, pool, cnt, B, K, mode, pos_score, pool_score, ws, stream, &s_tail))
        return rc;
    return pool_step_bwd(tb, gr, sample, weight, pool, cnt, B, K, mode, alpha, weight_sum, pos_score, pool_score, loss, ws,
                         stream, (s_tail.kind == 1 || s_tail.kind == 3) ? &s_tail : nullptr);
}
