// dp_tiles_stats.h -- the statistics recorder of the tiled fill (dp_tiles.hip: tile_body, pg_fill_tiles_flow).
//
// A statistics build (-DPG_TILE_STATS: tools/build_stamps.sh, never shipped) counts tiles, steps by kind, far fetches and the
// cycles of the prologue, the steps and the waits, summed over all tiles of a job, in 64-bit counters at the TAIL of the job's
// trace buffer, which a fill does not use; tools/probe_tile_stats.py reads the layout below out of this file (with
// tools/pipe_stats.py's reader) and prints a downloaded buffer.  This header is the only place that knows the switch: without it
// every recording point below expands to nothing and the kernels' code is the product's.
// The kernel says WHAT happens where; what is counted, where it is kept and where it goes is here.
#pragma once
#include "dp_device.h"

// ---- the trace tail: PG_TS_COUNTERS 64-bit counters from int PG_TS_FIRST(n3) of the buffer's n3 = 3 * (Lx + Ly) ints ----------
// Only jobs with n3 >= PG_TS_MIN_INTS record anything.  The counters begin PG_TS_BACK ints before the buffer's end, or one more
// where that is an odd int (the buffer is 8-byte aligned, n3 may be odd): a tail that the banded kernel's recorder
// (dp_pipe_stats.h) leaves alone.
#define PG_TS_MIN_INTS 4096
#define PG_TS_BACK 64
#define PG_TS_ALIGN 2
#define PG_TS_COUNTERS 18
#define PG_TS_FIRST(n3) (((n3) - PG_TS_BACK) & ~(PG_TS_ALIGN - 1))
// a tile (tile_body): how many, the cycles of their prologues, of the whole body
#define PG_TS_TILES 0
#define PG_TS_PROLOGUE 1
#define PG_TS_TILE_CYCLES 8
// steps with an active cell by kind (PG_TS_KINDS: 0 simple, 1 near, 2 loops -- dp_tiles.hip's header), and their cycles
#define PG_TS_KINDS 3
#define PG_TS_STEPS_SIMPLE 2
#define PG_TS_STEPS_NEAR 3
#define PG_TS_STEPS_LOOPS 4
#define PG_TS_CYCLES_SIMPLE 5
#define PG_TS_CYCLES_NEAR 6
#define PG_TS_CYCLES_LOOPS 7
// a tile of the dataflow schedule (pg_fill_tiles_flow), cycles: waiting for whole diagonals (the watermark), for the neighbours,
// acquire + tile body, release
#define PG_TS_WAIT_DIAGONALS 9
#define PG_TS_WAIT_NEIGHBOURS 10
#define PG_TS_ACQUIRE_TILE 11
#define PG_TS_RELEASE 12
// a block of the lagged start, cycles: waiting for the neighbours' progress, acquire + halo block + line block
#define PG_TS_LAG_WAIT 13
#define PG_TS_LAG_HALO 14
// loops steps: those with a fetch from beyond the LDS window (tile, halo, far lines), such fetches of the busiest lane summed over
// those steps, (left, right) edge pairs of the busiest lane summed over all loops steps
#define PG_TS_FAR_STEPS 15
#define PG_TS_FAR_FETCHES 16
#define PG_TS_PAIRS 17

#ifdef PG_TILE_STATS
namespace {
// what a wave counts over one tile
struct TileStats {
    unsigned long long steps[PG_TS_KINDS], cycles[PG_TS_KINDS];
    unsigned far, far_before, far_steps, far_max, pairs_max;       // far: fetches of this lane so far; far_before: ... at the step's start
    unsigned long long t_begin, t_loop, t_step, t_wait0, t_wait1;   // the clock at the tile's start, its step loop's, the step's, around a lagged block's wait
    int kind;                                                       // of the step in hand; -1: no active cell
};

__device__ __forceinline__ int pg_ts_wave_max(int v) {
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o));
    return v;
}
// the job's counters (n3 ints of trace buffer), or null for a job too short to have any
__device__ __forceinline__ unsigned long long *pg_ts_out(const PgDevJob *job, int n3) {
    return n3 >= PG_TS_MIN_INTS ? (unsigned long long *)(job->trace + PG_TS_FIRST(n3)) : nullptr;
}
// a tile ends (lane 0)
__device__ __forceinline__ void pg_ts_write_tile(const PgDevJob *job, int n3, const TileStats &ts) {
    if (unsigned long long *out = pg_ts_out(job, n3)) {
        atomicAdd(out + PG_TS_TILES, 1ull);
        atomicAdd(out + PG_TS_PROLOGUE, ts.t_loop - ts.t_begin);
        for (int k = 0; k < PG_TS_KINDS; ++k) { atomicAdd(out + PG_TS_STEPS_SIMPLE + k, ts.steps[k]); atomicAdd(out + PG_TS_CYCLES_SIMPLE + k, ts.cycles[k]); }
        atomicAdd(out + PG_TS_FAR_STEPS, (unsigned long long)ts.far_steps);
        atomicAdd(out + PG_TS_FAR_FETCHES, (unsigned long long)ts.far_max);
        atomicAdd(out + PG_TS_PAIRS, (unsigned long long)ts.pairs_max);
        atomicAdd(out + PG_TS_TILE_CYCLES, __builtin_amdgcn_s_memtime() - ts.t_begin);
    }
}
// a block of the lagged start is in LDS (lane 0)
__device__ __forceinline__ void pg_ts_write_lag(const PgDevJob *job, int n3, const TileStats &ts) {
    if (unsigned long long *out = pg_ts_out(job, n3)) {
        atomicAdd(out + PG_TS_LAG_WAIT, ts.t_wait1 - ts.t_wait0);
        atomicAdd(out + PG_TS_LAG_HALO, __builtin_amdgcn_s_memtime() - ts.t_wait1);
    }
}
// a tile of the dataflow schedule is released (lane 0): t0 taken from the queue, t1 the diagonals waited for, t2 the neighbours, t3
// the tile done
__device__ __forceinline__ void pg_ts_write_flow(const PgDevJob *job, unsigned long long t0, unsigned long long t1, unsigned long long t2,
                                                 unsigned long long t3) {
    if (unsigned long long *out = pg_ts_out(job, 3 * (job->Lx + job->Ly))) {
        atomicAdd(out + PG_TS_WAIT_DIAGONALS, t1 - t0);
        atomicAdd(out + PG_TS_WAIT_NEIGHBOURS, t2 - t1);
        atomicAdd(out + PG_TS_ACQUIRE_TILE, t3 - t2);
        atomicAdd(out + PG_TS_RELEASE, __builtin_amdgcn_s_memtime() - t3);
    }
}
}  // namespace

// ---- the recording points, statistics build.  `ts` is the tile's TileStats ----
#define PG_TS_CLOCK(name) const unsigned long long name = __builtin_amdgcn_s_memtime()
#define PG_TS_TILE_BEGIN TileStats ts = {}; ts.t_begin = __builtin_amdgcn_s_memtime()
#define PG_TS_LOOP_BEGIN ts.t_loop = __builtin_amdgcn_s_memtime()
#define PG_TS_TILE_END(job, n3) do { if (threadIdx.x == 0) pg_ts_write_tile(job, n3, ts); } while (0)
// a block of the lagged start: the wait for the neighbours' progress lies between the first two
#define PG_TS_LAG_WAIT_BEGIN ts.t_wait0 = __builtin_amdgcn_s_memtime()
#define PG_TS_LAG_WAIT_END ts.t_wait1 = __builtin_amdgcn_s_memtime()
#define PG_TS_LAG_END(job, n3) do { if (threadIdx.x == 0) pg_ts_write_lag(job, n3, ts); } while (0)
// a step: counted by the kind of its code path if the wave has an active cell (all three arguments are per lane)
#define PG_TS_STEP_BEGIN do { ts.t_step = __builtin_amdgcn_s_memtime(); ts.kind = -1; } while (0)
#define PG_TS_STEP_KIND(active, simple, near) \
    (ts.kind = __builtin_amdgcn_ballot_w64((active) && !(simple)) == 0 ? 0 : (__builtin_amdgcn_ballot_w64((active) && !(near)) == 0 ? 1 : 2))
#define PG_TS_STEP_END do { if (ts.kind >= 0) { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); const unsigned long long dt_ = __builtin_amdgcn_s_memtime() - ts.t_step; \
    for (int k_ = 0; k_ < PG_TS_KINDS; ++k_) if (k_ == ts.kind) { ++ts.steps[k_]; ts.cycles[k_] += dt_; } } } while (0)
// a loops step: `pairs` (left, right) edge pairs in this lane; a fetch of this lane went beyond the LDS window; the step's
// loops are through -- the wave's largest counts are what the step cost
#define PG_TS_LOOPS_BEGIN(pairs) do { ts.far_before = ts.far; ts.pairs_max += pg_ts_wave_max(pairs); } while (0)
#define PG_TS_FAR_FETCH (++ts.far)
#define PG_TS_LOOPS_END do { const int f_ = pg_ts_wave_max((int)(ts.far - ts.far_before)); ts.far_max += f_; ts.far_steps += f_ > 0; } while (0)
// a tile of the dataflow schedule
#define PG_TS_FLOW_END(job, t0, t1, t2, t3) do { if (threadIdx.x == 0) pg_ts_write_flow(job, t0, t1, t2, t3); } while (0)

#else  // the product: nothing is recorded
#define PG_TS_CLOCK(name)
#define PG_TS_TILE_BEGIN
#define PG_TS_LOOP_BEGIN
#define PG_TS_TILE_END(job, n3)
#define PG_TS_LAG_WAIT_BEGIN
#define PG_TS_LAG_WAIT_END
#define PG_TS_LAG_END(job, n3)
#define PG_TS_STEP_BEGIN
#define PG_TS_STEP_KIND(active, simple, near)
#define PG_TS_STEP_END
#define PG_TS_LOOPS_BEGIN(pairs)
#define PG_TS_FAR_FETCH
#define PG_TS_LOOPS_END
#define PG_TS_FLOW_END(job, t0, t1, t2, t3)
#endif
