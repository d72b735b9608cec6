// dp_pipe_stats.h -- the statistics recorder of pg_fill_pipe (dp_pipe.hip and its dp_pipe_*.inc parts).
//
// A statistics build (-DPG_PIPE_STATS: tools/build_stamps.sh, never shipped) counts steps, cycles and waits per wave and writes
// them to the TAIL of the job's trace buffer, which a fill does not use; tools/pipe_stats.py reads the layout below out of this
// file and decodes a downloaded buffer.  This header is the only place that knows the statistics switches:
//   PG_PIPE_STATS          the recorder as a whole; without it every recording point below expands to nothing, PipeSmem and
//                          WaveCtx carry no member of it, and the kernel's code is the product's
//   PG_STAT_CLASS=c        the class whose steps the phase stamps of the kernel's step() cover (default 0)
//   PG_AS_BUCKETS          lean assist waves: keep the cycle buckets 2..7 where the reasons for the general code are written otherwise
//   PG_ASSIST_RUNS_ONLY    large-table assist waves: count only diagonals that directly follow the wave's previous one
// The kernel's parts say WHAT happens where (PG_ST, POLL, PSTAMP, ASTAMP, the step macros); what is counted, where it is kept
// and where it goes is here.
#pragma once
#include "dp_kcommon.h"

// ---- the trace tail: int offsets, counted BACK from the buffer's end n3 = 3 * (Lx + Ly) ints ----------------------------------
// Only jobs with n3 >= PG_ST_MIN_INTS record anything: their last PG_ST_RESERVE ints belong to the regions below.
#define PG_ST_MIN_INTS 4096
#define PG_ST_RESERVE 1200
#define PG_ST_WAVES 4              // compute waves
#define PG_ST_ASSIST_WAVES 3
static_assert(PG_ST_ASSIST_WAVES == PG_PIPE_ASSIST, "one region per assist wave");
// cycle counts are written shifted right: the phase stamps and the run records' clocks by PG_ST_PHASE_SHIFT, every other by PG_ST_CYCLE_SHIFT
#define PG_ST_PHASE_SHIFT 4
#define PG_ST_CYCLE_SHIFT 8
// phase stamps, per compute wave: [0] steps of class PG_STAT_CLASS with cells, [1 + k] cycles / 16 of phase k -- flow control,
// lds wait + dpp, descriptor request + hand-over, compute, commit, carry + prefetch, loop edge
#define PG_ST_PHASE_BACK 200
#define PG_ST_PHASE_STRIDE 12
#define PG_ST_PHASE_FIELDS 8
// steps and cycles by class, per compute wave: [c] steps of class c with cells, [5 + c] their cycles / 256 (c = 0..4; class 5 runs count as 4)
#define PG_ST_CLASS_BACK 400
#define PG_ST_CLASS_STRIDE 12
#define PG_ST_CLASS_FIELDS 10
// wide-step buckets, per compute wave, cycles / 256: loader and neighbour flags, shift + records + operands off the wide ring,
// L2 operands, arithmetic + stores + flag
#define PG_ST_WIDE_BACK 600
#define PG_ST_WIDE_STRIDE 4
#define PG_ST_WIDE_FIELDS 4
// waits by kind (the `kind` of POLL / POLLX: 1 loader rows, 2 loader columns, 3 downstream (ring row reuse), 4 upstream (row above),
// 5 descriptor window, 6 far: all waves 8 steps behind, 7 rendezvous, 8 assist wave; 0, 5, 6, 7 and 9 also carry what the
// hand-scheduled loop counts itself: pg_stats_hot_loop), per compute wave: [kind] count, [10 + kind] cycles / 256
#define PG_ST_WAIT_BACK 800
#define PG_ST_WAIT_STRIDE 20
#define PG_ST_WAIT_FIELDS 20
// assist waves, per wave: [0] diagonals staged, [1 + k] cycles / 256 of bucket k (0..11), [13] diagonals that went to the general
// code whole, [14] passes that held two diagonals, [15] diagonals with cells staged by the general code; lean waves without
// PG_AS_BUCKETS: [3 + k] passes sent to the general code for reason k (slots, site shape, other side, cell shape / site 0,
// recent operand off the ring, pool)
#define PG_ST_ASSIST_BACK 1000
#define PG_ST_ASSIST_STRIDE 16
#define PG_ST_ASSIST_FIELDS 16
#define PG_ST_ASSIST_WHY 3
#define PG_ST_ASSIST_WHYS 6
// hardware ids, one HW_ID register per wave of the workgroup (compute 0-3, assist 4-6, loader 7)
#define PG_ST_HWID_BACK 1100
#define PG_ST_HWID_FIELDS 8
// per-run records of the hand-scheduled loop, in FRONT of the reserve: the region starts at n3 / DEN * NUM rounded up to ALIGN
// ints, with one slot counter per compute wave; PG_ST_RUN_HEAD ints further on, record (slot, wave) at 4 * (4 * slot + wave):
// first diagonal, diagonal the loop stopped in front of (bit 30: it left after 48 looks at the upstream flag), clock at entry / 16,
// clock at exit / 16
#define PG_ST_RUN_NUM 3
#define PG_ST_RUN_DEN 4
#define PG_ST_RUN_ALIGN 16
#define PG_ST_RUN_HEAD 16
#define PG_ST_RUN_INTS 4
#define PG_ST_RUN_BASE(n3) (((n3) / PG_ST_RUN_DEN * PG_ST_RUN_NUM + (PG_ST_RUN_ALIGN - 1)) & ~(PG_ST_RUN_ALIGN - 1))
#define PG_ST_RUN_CAP(n3) (((n3) - PG_ST_RESERVE - PG_ST_RUN_BASE(n3) - PG_ST_RUN_HEAD) / (PG_ST_RUN_INTS * PG_ST_WAVES))

// the strips of a job share its trace buffer: only the strip named in the debug flags' bits 12-15 records
#define PG_STATS_MINE(job, flags) (!(job)->is_strip || (job)->strip_row0 / PG_STRIP_ROWS == (int)(((flags) >> 12) & 15u))

#ifdef PG_PIPE_STATS
#ifndef PG_STAT_CLASS
#define PG_STAT_CLASS 0
#endif
namespace {
// what a compute wave counts, in the kernel and -- as WaveCtx::st -- in its run functions
struct PipeWaveStats {
    long long cls_t[PG_ST_CLASS_FIELDS / 2], poll_t[PG_ST_WAIT_FIELDS / 2], w[PG_ST_WIDE_FIELDS];        // cycles: steps by class, waits by kind, wide-step buckets
    int cls_n[PG_ST_CLASS_FIELDS / 2], poll_n[PG_ST_WAIT_FIELDS / 2];
};
// the phase stamps of the kernel's step(): they never leave the kernel
struct PipePhaseStats {
    long long acc[PG_ST_PHASE_FIELDS], t;
    int n;
    bool on;
};
// what an assist wave counts (poll_t / poll_n only so that POLL is the compute waves')
struct PipeAssistStats {
    long long poll_t[10];
    int poll_n[10];
    long long t[PG_ST_ASSIST_FIELDS - 4], t0;                         // cycle buckets, the clock at the last ASTAMP
    int n, gen, pairs, cells, why[PG_ST_ASSIST_WHYS];
    bool on;                                     // (PG_ASSIST_RUNS_ONLY) the diagonal in hand counts
    int prev;
};

// workgroup start: the slot counters of the per-run records, and which SIMD / CU every wave landed on
__device__ __forceinline__ void pg_stats_begin(const PgDevJob *job, unsigned flags, int tid) {
    // (only where a record fits: in a buffer of fewer than ~4,930 ints the counters would lie among the tail's regions)
    if (tid < PG_ST_WAVES && PG_ST_RUN_CAP(3 * (job->Lx + job->Ly)) > 0 && 3 * (job->Lx + job->Ly) >= PG_ST_MIN_INTS && PG_STATS_MINE(job, flags))
        ((PG_GLOBAL int *)job->trace)[PG_ST_RUN_BASE(3 * (job->Lx + job->Ly)) + tid] = 0;
    if ((tid & 63) == 0 && 3 * (job->Lx + job->Ly) >= PG_ST_MIN_INTS && PG_STATS_MINE(job, flags)) {
        unsigned hwid;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hwid));
        ((PG_GLOBAL int *)job->trace)[3 * (job->Lx + job->Ly) - PG_ST_HWID_BACK + (tid >> 6)] = (int)hwid;
    }
}

// a compute wave leaves the kernel (lane 0)
__device__ __forceinline__ void pg_stats_write_wave(const PgDevJob *job, unsigned flags, int n3, int wave, const PipeWaveStats &st, const PipePhaseStats &ph) {
    if (n3 >= PG_ST_MIN_INTS && PG_STATS_MINE(job, flags)) {
        PG_GLOBAL int *o = (PG_GLOBAL int *)job->trace + n3 - PG_ST_PHASE_BACK + PG_ST_PHASE_STRIDE * wave;
        o[0] = ph.n;
        for (int k = 0; k < PG_ST_PHASE_FIELDS - 1; ++k) o[1 + k] = (int)(ph.acc[k] >> PG_ST_PHASE_SHIFT);
        PG_GLOBAL int *q = (PG_GLOBAL int *)job->trace + n3 - PG_ST_CLASS_BACK + PG_ST_CLASS_STRIDE * wave;
        for (int c = 0; c < PG_ST_CLASS_FIELDS / 2; ++c) { q[c] = st.cls_n[c]; q[PG_ST_CLASS_FIELDS / 2 + c] = (int)(st.cls_t[c] >> PG_ST_CYCLE_SHIFT); }
        PG_GLOBAL int *u = (PG_GLOBAL int *)job->trace + n3 - PG_ST_WIDE_BACK + PG_ST_WIDE_STRIDE * wave;
        for (int c = 0; c < PG_ST_WIDE_FIELDS; ++c) u[c] = (int)(st.w[c] >> PG_ST_CYCLE_SHIFT);
        PG_GLOBAL int *v = (PG_GLOBAL int *)job->trace + n3 - PG_ST_WAIT_BACK + PG_ST_WAIT_STRIDE * wave;
        for (int c = 0; c < PG_ST_WAIT_FIELDS / 2; ++c) { v[c] = st.poll_n[c]; v[PG_ST_WAIT_FIELDS / 2 + c] = (int)(st.poll_t[c] >> PG_ST_CYCLE_SHIFT); }
    }
}

// an assist wave starts: everything counts, the first bucket's clock runs
__device__ __forceinline__ PipeAssistStats pg_stats_assist_begin() {
    PipeAssistStats s = {};
    s.on = true; s.prev = -100; s.t0 = __builtin_readcyclecounter();
    return s;
}
// an assist wave leaves the kernel (lane 0). `lean`: pipe_assist_lean, which runs for strips too and knows the general code's
// counters; the large-table waves write their diagonals and buckets only, and never asked which strip records (as before this
// header: no job with a large table is cut into strips, so the question does not come up for them)
__device__ __forceinline__ void pg_stats_write_assist(const PgDevJob *job, unsigned flags, int a, const PipeAssistStats &st, bool lean) {
    if (3 * (job->Lx + job->Ly) >= PG_ST_MIN_INTS && (!lean || PG_STATS_MINE(job, flags))) {
        PG_GLOBAL int *o = (PG_GLOBAL int *)job->trace + 3 * (job->Lx + job->Ly) - PG_ST_ASSIST_BACK + PG_ST_ASSIST_STRIDE * a;
        o[0] = st.n;
        for (int k = 0; k < PG_ST_ASSIST_FIELDS - 4; ++k) o[1 + k] = (int)(st.t[k] >> PG_ST_CYCLE_SHIFT);
        if (lean) {
            o[PG_ST_ASSIST_FIELDS - 3] = st.gen; o[PG_ST_ASSIST_FIELDS - 2] = st.pairs; o[PG_ST_ASSIST_FIELDS - 1] = st.cells;
#ifndef PG_AS_BUCKETS
            for (int k = 0; k < PG_ST_ASSIST_WHYS; ++k) o[PG_ST_ASSIST_WHY + k] = st.why[k];
#endif
        }
    }
}

// one run of the hand-scheduled loop (hot_run, lane 0 of the wave): its record, while the wave's slots last
__device__ __forceinline__ void pg_stats_write_run(const PgDevJob *job, unsigned flags, int n3, int tid, int wave, int d_in, int d_out, int k0,
                                                   long long t_in, long long t_out) {
    const int r0 = PG_ST_RUN_BASE(n3), cap = PG_ST_RUN_CAP(n3);
    if (cap > 0 && n3 >= PG_ST_MIN_INTS && (tid & 63) == 0 && PG_STATS_MINE(job, flags)) {
        PG_GLOBAL int *tb = (PG_GLOBAL int *)job->trace;
        const int slot = atomicAdd((int *)(tb + r0 + wave), 1);
        if (slot < cap) {
            PG_GLOBAL int *o = tb + r0 + PG_ST_RUN_HEAD + PG_ST_RUN_INTS * (slot * PG_ST_WAVES + wave);
            o[0] = d_in; o[1] = __builtin_amdgcn_readfirstlane(d_out) | ((k0 >> 16) ? 0x40000000 : 0); o[2] = (int)(t_in >> PG_ST_PHASE_SHIFT); o[3] = (int)(t_out >> PG_ST_PHASE_SHIFT);
        }
    }
}
// ... and what the loop counted itself (tools/gen_hot_asm.py): k0 = waits for the upstream wave | 48-look exits << 16, k1 = looks at
// the upstream flag, k2 = waits for the downstream wave | cycles / 256 of the 48-look exits << 16; `nd_run` diagonals in this run
__device__ __forceinline__ void pg_stats_hot_loop(PipeWaveStats &st, int k0, int k1, int k2, int nd_run) {
    st.poll_n[9] += k0 & 0xffff; st.poll_n[6] += k1; st.poll_t[9] += (long long)(k2 & 0xffff) << PG_ST_CYCLE_SHIFT; st.poll_n[5] += k0 >> 16; st.poll_t[5] += (long long)(k2 >> 16) << PG_ST_CYCLE_SHIFT; st.poll_n[0] += 1; st.poll_t[0] += (long long)nd_run << PG_ST_CYCLE_SHIFT;
}

}  // namespace

// ---- the recording points, statistics build.  `st` is the wave's PipeWaveStats / PipeAssistStats, `ph` the kernel's PipePhaseStats ----
#define PG_ST(...) __VA_ARGS__                                     // a statement of the recorder's
#define PG_ST_CLOCK(name) const long long name = __builtin_readcyclecounter()
#define PG_ST_SMEM long long far_limit;                            // PipeSmem: bytes of the job's score array
#define PG_ST_CTX PipeWaveStats st;                                // WaveCtx
#define WCTX_STATS(c) PipeWaveStats &st = (c).st
// a wait, timed and counted by kind
#define POLLX(p, need, kind) ([&] { const long long t0_ = __builtin_readcyclecounter(); const int v_ = __builtin_amdgcn_readfirstlane(poll_ge_out(p, need, PTAG(kind))); st.poll_t[kind] += __builtin_readcyclecounter() - t0_; ++st.poll_n[kind]; return v_; }())
#define POLL(p, need, kind) ([&] { const long long t0_ = __builtin_readcyclecounter(); const int v_ = poll_ge(p, need, PTAG(kind)); st.poll_t[kind] += __builtin_readcyclecounter() - t0_; ++st.poll_n[kind]; return v_; }())
// phase k of the kernel's step() ends here; bucket k of an assist wave's pass ends here (12: the loop's top, bucket 0)
// (PG_ST_PHASE_BEGIN: the kernel's loop is about to take the diagonal of descriptor dA; its steps count if it is of class PG_STAT_CLASS)
#define PG_ST_PHASE_BEGIN(dA, row) do { ph.on = ((dA).s4 & 15) == PG_STAT_CLASS && __any((row) <= (dA).y && (row) >= (dA).x); ph.t = __builtin_readcyclecounter(); if (ph.on) ph.n += 2; } while (0)
#define PSTAMP(k) do { const long long t_ = __builtin_readcyclecounter(); if (ph.on) ph.acc[k] += t_ - ph.t; ph.t = t_; } while (0)
#define ASTAMP(k) do { const long long t_ = __builtin_readcyclecounter(); if (st.on) st.t[(k) == 12 ? 0 : (k)] += t_ - st.t0; st.t0 = t_; } while (0)
// a step of the C++ renderings (hot_run, step()): counted by class if the wave has a cell on the diagonal
#define PG_ST_STEP_BEGIN(row, lo, hi) PG_ST_CLOCK(st_step0); const bool st_has = __any((row) <= (hi) && (row) >= (lo))
#define PG_ST_STEP_END(cls) do { if (st_has) { const long long dt = __builtin_readcyclecounter() - st_step0; for (int c = 0; c < 5; ++c) if (c == (cls)) { st.cls_t[c] += dt; ++st.cls_n[c]; } } } while (0)
// a wide step (class 4 / 5, counted as class 4) that began at st_step0; with its buckets' clocks st_t1..st_t3 where it has them
#define PG_ST_WIDE_END(mine) do { if (mine) { st.cls_t[4] += __builtin_readcyclecounter() - st_step0; ++st.cls_n[4]; } } while (0)
#define PG_ST_WIDE_END_BUCKETS(mine) do { if (mine) { const long long st_t5 = __builtin_readcyclecounter(); st.cls_t[4] += st_t5 - st_step0; ++st.cls_n[4]; \
    st.w[0] += st_t1 - st_step0; st.w[1] += st_t2 - st_t1; st.w[2] += st_t3 - st_t2; st.w[3] += st_t5 - st_t3; } } while (0)
// far reads: a cell outside the job's score array sets the abort flag instead of being read
// (PG_ST_FAR_GUARD: `bad` is an expression over PG_ST_FAR_OUTSIDE(ask); the function returns without reading)
#define PG_ST_FAR_OUTSIDE(a) ((a).need && ((a).boff < 0 || (a).boff + 24 > far_lim_))
#define PG_ST_FAR_GUARD(bad, tag) do { const long long far_lim_ = PM.far_limit; if (__builtin_amdgcn_ballot_w64(bad) != 0) { if (PM.abort_flag == 0) PM.abort_flag = (tag); return; } } while (0)
#define PG_ST_FAR_WANTED(a, tag) ([&] { const long long far_lim_ = PM.far_limit; const bool bad_ = PG_ST_FAR_OUTSIDE(a); if (__builtin_amdgcn_ballot_w64(bad_) != 0 && PM.abort_flag == 0) PM.abort_flag = (tag); return (a).need && !bad_; }())
// (PG_ASSIST_RUNS_ONLY: only diagonals that directly follow the wave's previous one -- the inside of a class 2 run, where the assist
// waves are what the compute waves wait for -- are counted; otherwise the idle time between runs dominates the averages)
#ifdef PG_ASSIST_RUNS_ONLY
#define PG_ST_ASSIST_NEXT(q_d) (st.on = (q_d) == st.prev + PNA)
#else
#define PG_ST_ASSIST_NEXT(q_d) ((void)0)
#endif

#else  // the product: nothing is recorded
#define PG_ST(...)
#define PG_ST_CLOCK(name)
#define PG_ST_SMEM
#define PG_ST_CTX
#define WCTX_STATS(c)
#define POLLX(p, need, kind) __builtin_amdgcn_readfirstlane(poll_ge_out(p, need, PTAG(kind)))
#define POLL(p, need, kind) poll_ge(p, need, PTAG(kind))
#define PG_ST_PHASE_BEGIN(dA, row)
#define PSTAMP(k)
#define ASTAMP(k)
#define PG_ST_STEP_BEGIN(row, lo, hi)
#define PG_ST_STEP_END(cls)
#define PG_ST_WIDE_END(mine)
#define PG_ST_WIDE_END_BUCKETS(mine)
#define PG_ST_FAR_GUARD(bad, tag)
#define PG_ST_FAR_WANTED(a, tag) ((a).need)
#endif
