// Launch plan of the Adam kernels (adam.hip): which row kernel runs for a row width, an id list and a step, with which rows per
// workgroup, access width, sweep window and rider workgroups.  Plain host code: no device code, no HIP calls, no environment --
// adam.hip reads MKB_ADAM_SWEEP and hands its value in; tests/test_host_adam_routes.py asks these very functions which leaf a case
// of tests/util_adam_routes.py takes.
#pragma once
#include <stdint.h>
#include <algorithm>

namespace mkb {

// workgroup size of the catch-up / advance kernel (the sampler's filter and draw blocks that ride it are sized by it too)
// 512 lanes: one 2000-float row per workgroup, two workgroups per CU (107 VGPRs): their phases -- ownership exchange, loads, replay,
// stores -- interleave.  Round 4, same box, 1024 -> 512 lanes: headline step 0.2273 -> 0.2242 ms, WN18RR 0.1302 -> 0.1262, YAGO3-10
// 0.1933 -> 0.1862 (256 lanes: better still for YAGO3-10's long replays, worse at the headline; variants built with
// -DMKB_CATCH_THREADS / -DMKB_REPLAY_UNROLL by tools/kbench.py)
#ifndef MKB_CATCH_THREADS
#define MKB_CATCH_THREADS 512
#endif
constexpr int kCatchThreads = MKB_CATCH_THREADS;
#ifndef MKB_REPLAY_UNROLL
#define MKB_REPLAY_UNROLL 4
#endif
constexpr int kReplayUnroll = MKB_REPLAY_UNROLL;  // pending zero-gradient steps replayed side by side

constexpr int kAdamHostThreads = 256;  // workgroup size of adam_kernel, adam_multi_kernel, adam_rows_flush_kernel, adam_rows_step_kernel
constexpr int64_t kAdamDenseMaxBlocks = 2048, kAdamRiderMaxBlocks = 1024;  // grid-stride caps: a dense launch | a rider's workgroups

// Sweep.  Exact dense Adam moves every parameter every step, so the replay's arithmetic is N x D element-steps per step no
// matter when it happens (measured: ~85 ns per wave and pending step at 4 elements per lane: WN18RR +16 us, FB15k-237
// +12 us, YAGO3-10 ~40 us per launch if spread evenly).  It is NOT spread evenly when entities are rare: a YAGO3-10 entity
// that only the random pool reaches waits ~1,500 steps in the tail, its chain is serial, and the launch lasts as long as
// its longest chain (99 us measured).  So when the mean gap N / rows-per-step is large, each per-step launch also visits
// a moving window of min(N / period, rows-of-this-launch) rows: every row is brought up to date at least once per
// max(period, N / rows-per-launch) steps (the window never exceeds the launch's own row count, so for N > period * rows the
// bound is N / rows; the window's start is a function of the step and of THAT launch's window, so launches with different row
// counts -- a catch-up of a few ids between two training steps -- move it unevenly: a latency aid, not a guarantee).  Same
// arithmetic, same results bit for bit (every pending step of every row is replayed exactly once, whenever that happens);
// cost: the window's rows x (p, m, v) in + out.  YAGO3-10: 99 -> 64 us per launch, step 0.268 -> 0.211 ms; WN18RR / FB15k-237
// (mean gap 18 / 6 steps, every entity is a positive often enough): no gain, so no sweep.
// Round 5, with the replay's per-step round trips gone and in runs long enough for the gaps to reach their steady state (1,500
// steps): WN18RR's launch 36.5 us without a sweep, 31.3-31.9 with a period of 24-48 (step 0.1193 -> 0.1144 ms), 32.5 at 128;
// YAGO3-10 91.8 without, 53.1 / 54.5 / 65.1 / 79.0 at 32 / 64 / 128 / 256; FB15k-237 37.7 without, 37.7-39.1 with.  Hence: a
// period of 32 from a mean gap of 12 steps on.
constexpr int kSweepPeriod = 32, kSweepMinGap = 12;

// workgroups that stream a dense tensor of n floats: `threads` lanes x float4, grid-stride over 1 .. max_blocks of them
inline int64_t adam_dense_blocks(int64_t n, int threads, int64_t max_blocks) {
    return std::min(std::max(((n >> 2) + threads - 1) / threads, (int64_t)1), max_blocks);
}

enum class AdamRowsCall {
    Advance,  // mkb_adam_rows_advance / mkb_adam_rows_advance_generate: catch-up, advance form, flush
    Step,     // mkb_adam_rows_step
};

enum class AdamRowsKernel {
    CatchupUnroll,  // adam_rows_catchup_kernel<kReplayUnroll>: rows wait many steps between visits
    CatchupLean,    // adam_rows_catchup_kernel<1>: short gaps, few registers
    Flush,          // adam_rows_flush_kernel: every row of the table, one 256-lane workgroup per row, one step at a time
    Step,           // adam_rows_step_kernel: the real step of the listed rows
};

struct AdamRowsShape {
    int64_t D;         // row width
    bool aligned16;    // param, grad (where given), exp_avg and exp_avg_sq all start on a 16-byte boundary
    int64_t rows;      // rows the call lists (ownership entries and local ids together; the whole table for a flush); 0 = nothing pending
    int64_t n_table;   // rows of the table
    int64_t step;      // the step the rows are brought to (Advance) or that is applied (Step)
    bool listed;       // the rows come from an id list (or the batch's pool | heads | tails segments), not "the whole table"
    int forced_sweep;  // MKB_ADAM_SWEEP as a value: a period > 0, 0 = no sweep, < 0 = unset (the built-in rule)
    int64_t rider_n;   // floats of the dense rider (0 = none)
};

// What drives the launch: kernel, threads, row_blocks, rider_blocks (the grid and the kernel launched), and for the catch-up kernel
// vec4, rows_per_block, rows_listed, sweep_start and table_bound, which adam.hip copies into the kernel's arguments (the flush
// kernel reads vec4, rows_listed and table_bound of them, the step kernel table_bound).  What only DESCRIBES the launch, for the
// tests' case table: epl, access, lanes_per_row, passes, sweep_rows, and vec4 of a Step plan -- the flush and step kernels take
// their access width from D themselves and stride by 256 lanes x epl; these fields restate that and must be kept in step with
// adam.hip by hand.
struct AdamRowsPlan {
    AdamRowsKernel kernel;
    int threads;          // lanes per workgroup of that kernel (its rider workgroups included)
    int vec4;             // rows are read as float4 per lane (D % 4 == 0; the replay kernels also need 16-byte aligned arrays)
    int epl;              // elements per lane and pass: 4 | 2 (replay kernels), 4 | 1 (step kernel)
    int access;           // floats per memory access: 4 | 2 | 1 (an odd D takes the replay's 2 elements per lane one at a time)
    int rows_per_block;   // catch-up kernel: power of two <= 8 at 512 lanes; 1 elsewhere
    int lanes_per_row;    // threads / rows_per_block
    int passes;           // ceil(D / (epl * lanes_per_row)): chunks a lane walks
    int64_t sweep_rows;   // rows of the moving window behind the listed ones (0 = no sweep)
    int64_t sweep_start;  // its first table row; it wraps past the end of the table
    int64_t rows_listed;  // rows + sweep_rows
    int64_t row_blocks;   // workgroups that take rows
    int64_t rider_blocks; // workgroups behind them that stream the rider
    int64_t table_bound;  // what the kernel checks ids against (0 = no id list to check)
};

inline AdamRowsPlan plan_adam_rows(AdamRowsCall call, const AdamRowsShape &s) {
    AdamRowsPlan P{};
    if (call == AdamRowsCall::Step) {
        P.kernel = AdamRowsKernel::Step;
        P.threads = kAdamHostThreads;
        P.vec4 = (s.D & 3) == 0;
        P.epl = P.access = P.vec4 ? 4 : 1;
        P.rows_per_block = 1;
        P.lanes_per_row = P.threads;
        P.rows_listed = P.row_blocks = s.rows;
        P.table_bound = s.n_table;  // (ids past the table are skipped, not stepped out of bounds)
    } else {
        const int64_t n_table = s.listed ? s.n_table : 0;  // (a flush walks the whole table anyway)
        int64_t rows = s.rows;
        if (rows > 0 && n_table > 0 && s.step > 0) {
            if (s.forced_sweep > 0) P.sweep_rows = (n_table + s.forced_sweep - 1) / s.forced_sweep;
            else if (s.forced_sweep < 0 && n_table >= (int64_t)kSweepMinGap * rows)
                P.sweep_rows = std::min((n_table + kSweepPeriod - 1) / kSweepPeriod, rows);
            if (P.sweep_rows > 0) P.sweep_start = ((s.step - 1) * P.sweep_rows) % n_table;
        }
        P.rows_listed = rows + P.sweep_rows;
        P.table_bound = n_table;
        P.vec4 = (s.D & 3) == 0 && s.aligned16;
        P.epl = P.vec4 ? 4 : 2;
        P.access = P.vec4 ? 4 : ((s.D & 1) == 0 ? 2 : 1);
        if (!s.listed && P.rows_listed > 0) {
            P.kernel = AdamRowsKernel::Flush;
            P.threads = kAdamHostThreads;
            P.rows_per_block = 1;
            P.row_blocks = P.rows_listed;
        } else {
            // mean gap between two visits of a row = table rows / rows a launch lists: short gaps take the lean replay
            const bool short_gaps = n_table > 0 && rows > 0 && n_table < (int64_t)kSweepMinGap * rows;
            P.kernel = short_gaps ? AdamRowsKernel::CatchupLean : AdamRowsKernel::CatchupUnroll;
            P.threads = kCatchThreads;
            // as many rows per workgroup as fit with one chunk per lane (whole waves per row): at 512 lanes 2000-float rows 1,
            // 1000-float rows 2, the 250-float rows of an 8-way dimension shard 8 -- short rows used to idle most of the lanes
            const int64_t lanes = ((s.D + P.epl - 1) / P.epl + 63) / 64 * 64;
            int rpb = 1;
            while (rpb < 16 && (int64_t)kCatchThreads / (rpb * 2) >= lanes) rpb *= 2;
            P.rows_per_block = rpb;
            P.row_blocks = (P.rows_listed + rpb - 1) / rpb;
        }
        P.lanes_per_row = P.threads / P.rows_per_block;
    }
    P.passes = (int)((s.D + (int64_t)P.epl * P.lanes_per_row - 1) / ((int64_t)P.epl * P.lanes_per_row));
    P.rider_blocks = s.rider_n > 0 ? adam_dense_blocks(s.rider_n, P.threads, kAdamRiderMaxBlocks) : 0;
    return P;
}

}  // namespace mkb
