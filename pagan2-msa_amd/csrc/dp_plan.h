// dp_plan.h -- the aligner's host-only planning (dp_plan.cpp): the environment switches, the plan of one job (band index,
// classes and wave schedule of the banded kernel, row strips, tiles, traceback boundaries), the kernel it is routed to, the
// descriptor words, dead-site compaction and the path replay.  Plain C++17, no HIP: dp_abi.hip stages and launches what this
// plans, and everything here runs (and is tested) without a device.
#pragma once
#include <algorithm>
#include <atomic>
#include <cstdint>
#include <thread>
#include <vector>

#include "../../include/pagan_dp.h"
#include "dp_device.h"
#include "dp_band.h"

namespace pgplan {

// Every PAGAN_DP_* variable the aligner's host code reads, parsed (INTEGRATION.md lists them by these names).  Read once at an
// entry point and passed down: the create-time ones by pagan_batch_create and the host-only pagan_dp_debug_* calls, the
// run-time ones by pagan_batch_run, `rerun` by pagan_batch_fetch -- tests flip variables between calls.
struct DpSwitches {
    // ---- create-time ----
    enum Fill { FILL_PIPE, FILL_RING, FILL_TILES } fill = FILL_PIPE;   // FILL: =ring the barrier-per-diagonal LDS kernel for the banded jobs, =tiles no banded jobs
    int bp = 1;                          // BP: 1 back-pointers by pg_backptr, =verify 2 (pg_backptr compares), =fill 0 (the ring kernel writes its own)
    uint32_t debug_flags = 0;            // DEBUG_FLAGS: bits 8-15 of the kernels' flag word
    enum Wide { WIDE_STRIPS, WIDE_TILES, WIDE_WAVEFRONT } wide = WIDE_STRIPS;   // WIDE: unset / =strips, =wavefront, anything else (=tiles)
    bool force_global_wavefront = false; // FORCE_GLOBAL_WAVEFRONT (set at all): every job on the one-workgroup HBM wavefront
    bool compact = true;                 // COMPACT=0: dead sites stay in
    bool strip_spread = true;            // STRIP_SPREAD=0: a job's strips on one XCD (round 4's placement)
    int strip_states = 16;               // STRIP_STATES: the largest model that runs as row strips
    int strip_sites = 56;                // STRIP_SITES: most multi-edge sites on a strip's diagonal
    bool strip_term = false;             // STRIP_TERM (set at all): a strip's diagonals with a cell of the first / last column take the C++ step
    enum Tiles { TILES_FLOW, TILES_WATERMARK, TILES_NOLAG, TILES_LAUNCHES } tiles = TILES_FLOW;   // TILES
    bool canary = false;                 // CANARY (not 0): guard words behind every region of the arena; =0x...: that pattern
    unsigned canary_word = 0x5ca1ab1eu;
    bool wide7 = true;                   // WIDE7=0: every wide run stays with the four compute waves
    enum Hist { HIST_ON, HIST_NARROW, HIST_OFF } hist = HIST_ON;       // HIST: =narrow no interval across a wide run, =0 no far histories
    bool three = true;                   // THREE=0: no third pass for three-edge sites
    int after_wide = 3;                  // AFTER_WIDE=reach: PG_PIPE_REACH general steps behind a wide diagonal, as before round 5
    int plan_threads = 1;                // PLAN_THREADS: pagan_dp_debug_plan's plan over several threads
    // ---- run-time ----
    enum ScoreCheck { CHECK_DEFAULT, CHECK_OFF, CHECK_ALL } score_check = CHECK_DEFAULT;   // SCORE_CHECK: =0, =all
    bool follow = true;                  // FOLLOW=0: no follower workgroups behind the banded fill
    // ---- fetch-time ----
    bool rerun = true;                   // RERUN=0: a failed path / score check is reported at once
    // ---- wherever it is read ----
    bool verbose = false;                // VERBOSE (set at all)
    bool plan_profile = false;           // PLAN_PROFILE (set at all; looked at once per process)
    static DpSwitches read();
};

// (PLAN_PROFILE) "<prefix><what> x.xx ms" on stderr for the time since the last lap
struct Lap {
    const char *prefix;
    bool on;
    double t_last;
    Lap(const char *prefix_, bool on_);
    void operator()(const char *what);
};

// The fill kernel a job gets; the codes are pagan_dp_debug_route's.
enum Route { PIPE_SMALL = 0, PIPE_BIG = 1, TILES = 2, WAVEFRONT = 3, STRIPS = 4 };

// One row strip of a wide job (dp_pipe.hip, strip_feeder has the scheme): rows r0..r1, descriptors of the diagonals d0..d1-1.
struct StripPlan {
    int r0 = 0, r1 = 0, d0 = 0, d1 = 0, feed_wave = -1, col_first = 0;
    std::vector<int> psc;        // [d1 - d0 + 1][8] (one entry of padding), as PgDevJob::psc
    std::vector<int> sched;      // as PgDevJob::sched
};

struct HostJob {
    const pagan_graph *L, *R;
    int Lx, Ly;
    DiagIndex dx;
    bool ring_ok = false;        // fits the LDS-staged narrow-band kernel
    std::vector<uint8_t> cls;    // per diagonal: how dp_pipe.hip computes it (empty: not a pipe job)
    std::vector<int> sched;      // dp_pipe.hip: awake intervals of the four compute waves (dp_device.h)
    std::vector<int> lead_req;   // dp_pipe.hip: per diagonal, what the downstream wave must have completed first
    std::vector<uint8_t> ring2;  // dp_pipe.hip: class 2 diagonals whose operands all lie in the ring
    // far histories (dp_pipe.hip, PipeSmem::hist; plan_far_hist): per site of either graph a flag byte, per diagonal
    // whether a reader or a writer of a history line has a cell on it; all empty when the job has none
    std::vector<uint8_t> hfL, hfR, hbit;
    std::vector<uint8_t> tbit;   // per diagonal: a three-edge site the lanes take in a third pass has a cell on it (empty: none)
    std::vector<int> tiles;      // dp_tiles.hip (jobs that are not ring_ok): tile row, tile column of every tile that may hold a cell
    std::vector<struct StripPlan> strips;   // dp_pipe.hip, row strips (jobs that are not ring_ok and qualify: plan_strips); empty otherwise
    int n_bound = 0;             // traceback boundaries (dp_device.h)
    std::vector<int> tb;         // [n_bound + 2] table offsets
    Route route = WAVEFRONT;     // route_of() over the fields above: what the grouping, pagan_dp_debug_route and the launches go by
};

// ---- dead sites (dp_plan.cpp has the reasoning) ----
struct CompactSide {
    std::vector<int> keep;       // compacted site -> caller's site
    std::vector<int> state, off, src, eid, slot;   // compacted graph arrays; slot: position of the edge in the caller's list of its site
    std::vector<float> w;
    pagan_graph g;
    int dead = 0;
    void build(const pagan_graph *o);
};
struct CompactJob {
    bool on = false;
    const pagan_graph *L0 = nullptr, *R0 = nullptr;   // the caller's graphs
    int64_t cells0 = 0;                               // the caller's in-band cells
    CompactSide l, r;
    std::vector<int> up, lo;
    pagan_band band;
};
// Dead sites out of one job: fills `cj` and points `eff` at the compacted graphs / band when the job qualifies (5 % dead
// sites or more, nothing validate_job would refuse).
void compact_job(const pagan_job &jb, bool allow, CompactJob *cj, pagan_job *eff);

// Checks and plans one job and sets its route.  allow_strips = false: a wide job never gets row strips (pagan_dp_align_batch's
// third attempt).  `threads`: the plan of ONE alignment over several host threads.
int validate_job(const pagan_job &jb, HostJob *hj, const DpSwitches &sw, bool allow_strips = true, int threads = 1);
Route route_of(const HostJob &hj, int n_states, const DpSwitches &sw);

// The per-diagonal descriptors pg_fill_pipe reads for a banded job (PgDevJob::psc: 8 words per diagonal + one entry of padding),
// from the job's plan.  `packed` holds 8 * (diagonals + 1) ints.
void pack_pipe_descriptors(const HostJob &hj, int n_states, const DpSwitches &sw, int *packed);

// The tile list of a batch's tiled jobs as the device reads it (dp_tiles.hip): {job, tile row, tile column, position of the
// tile above} ordered by row + column, then the positions of the tiles to the left, of the diagonal neighbours, then tile_off
// (first tile of tile anti-diagonal t; tile_off.back() = total).  *water: some job's tiles are no staircase.  Nothing for no jobs.
void build_tile_list(const std::vector<HostJob> &jobs, const std::vector<int> &which_tiled, std::vector<int> *tile_list,
                     std::vector<int> *tile_off, bool *water);

// The strips' launches: a strip is a device job of its own behind the batch's n, job-major (sdev: {job, strip}); swhich lists
// them in workgroup order (-1: padding) -- first the launch of the jobs whose model table fits LDS (grid[0] entries), then the
// others' (grid[1]) -- under either placement (spread: any XCD, by first diagonal; otherwise a job's strips on one XCD).
void order_strips(const std::vector<HostJob> &jobs, const std::vector<pagan_job> &eff, const std::vector<int> &which_striped, int n,
                  bool spread, std::vector<std::pair<int, int>> *sdev, std::vector<int> *swhich, int grid[2]);

// Host side of the traceback: the device's visited cells -> the reference's path (columns + used edges).
int replay(const HostJob &hj, const int *endcell, double endscore, const int *trace, bool verbose, pagan_result *out);

// Independent per-job host work (validation, diagonal index, plan, staging) over a few threads: a batch
// is a guide-tree level, up to hundreds of 1e5-site jobs.
template <class F> void parallel_jobs(int n, F f) {
    const int hw = (int)std::thread::hardware_concurrency();
    const int nt = std::max(1, std::min({n, hw > 0 ? hw : 1, 16}));
    if (nt == 1) { for (int k = 0; k < n; ++k) f(k); return; }
    std::atomic<int> next{0};
    std::vector<std::thread> pool;
    for (int t = 0; t < nt; ++t)
        pool.emplace_back([&] { for (int k = next++; k < n; k = next++) f(k); });
    for (auto &th : pool) th.join();
}

} // namespace pgplan
