// dp_abi.hip -- the C ABI of include/pagan_dp.h on top of the gfx950 kernels.
//
// Host work done here is bookkeeping only: what dp_plan.cpp validated and planned (the band's per-anti-diagonal index,
// the kernels' plans, every job's route) is staged into ONE device arena per batch and launched, and the device's list of
// visited path cells goes back through dp_plan.cpp's replay.
// There is no CPU fill or traceback here: without a HIP device every entry point fails.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <thread>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <condition_variable>
#include <mutex>
#include <new>
#include <type_traits>
#include <vector>

#include "dp_hip.h"
#include "host_anchors.h"
#include "host_graph.h"
#include "dp_plan.h"

using namespace pgplan;
using namespace pgdev;

template <int BLOCK> __global__ void pg_fill_wavefront(const PgDevJob *jobs, const int *which, unsigned flags);
template <bool TAB_LDS> __global__ void pg_fill_ring(const PgDevJob *jobs, const int *which, unsigned flags);
template <bool TAB_LDS, bool STRIP> __global__ void pg_fill_pipe(const PgDevJob *jobs, const int *which, unsigned flags, int n_fill);
__global__ void pg_fill_tiles(const PgDevJob *jobs, const int *tiles, unsigned flags);
__global__ void pg_fill_tiles_flow(const PgDevJob *jobs, const int *tiles, int n_tiles, int n_diag, int *flow, unsigned flags, int schedule);
__global__ void pg_end_corner(const PgDevJob *jobs, const int *tiles_gave_up);
__global__ void pg_backptr(const PgDevJob *jobs, const int *which, unsigned flags, int diags_per_block);
__global__ void pg_trace_spec(const PgDevJob *jobs);
__global__ void pg_trace_compose(const PgDevJob *jobs);
__global__ void pg_trace_emit(const PgDevJob *jobs);
__global__ void pg_trace_check(const PgDevJob *jobs, unsigned flags);
__global__ void pg_debug_poke_bp(const PgDevJob *jobs, int k, int i, int j, int vit, unsigned word);

unsigned pg_ring_lds_bytes();
unsigned pg_pipe_lds_bytes();        // (static LDS: reported, not passed at launch)
unsigned pg_pipe_block();
unsigned pg_tiles_lds_bytes();

extern "C" void pagan_fb_internal_release_cache();             // dp_fb.hip: the forward/backward arenas kept for the next pair

namespace {

#define HIP_TRY(expr) PG_HIP_CODE(expr, "pagan_dp", PAGAN_E_NODEVICE)

struct Arena {
    char *dev = nullptr;
    size_t size = 0;         // bytes the batch uses
    size_t cap = 0;          // bytes allocated (an arena taken from the pool may be larger)
};

// Device arenas are reused by the next batch on the same device: hipFree of a few GB costs 10-30 ms, and a level
// of a tree walk is followed by the next.  At most two idle arenas per device; pagan_dp_release_cache() frees them.
// Any idle arena that is large enough is taken; a miss allocates what the batch uses, and take_arena does the retry itself.
const SlabPolicy kArenaPolicy = {
    /* slack_mul, slack_add */ 0, 0, /* grow_div */ 0, /* max_idle */ 0, /* max_idle_per_device */ 2, /* max_idle_bytes */ 0,
    /* evict_smallest */ true, /* retry_drained */ false};
SlabPool arena_pool(kArenaPolicy);

// Streams and events of a batch, reused by the next batch on the same device (at most four idle sets per device).
struct GpuObjs {
    hipStream_t stream = nullptr, stream2 = nullptr;
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr}, evk[7] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    void destroy() {
        if (stream) (void)hipStreamDestroy(stream);
        if (stream2) (void)hipStreamDestroy(stream2);
        for (auto &e : ev) if (e) (void)hipEventDestroy(e);
        for (auto &e : evk) if (e) (void)hipEventDestroy(e);
        if (ev_fork) (void)hipEventDestroy(ev_fork);
        if (ev_join) (void)hipEventDestroy(ev_join);
    }
};
IdlePerDevice<GpuObjs> gpu_pool;
void destroy_objs(std::vector<std::pair<int, GpuObjs>> &drop) { for (auto &e : drop) { DeviceScope on(e.first); e.second.destroy(); } }

} // namespace

// (PAGAN_DP_CANARY: guard words behind every region of the arena -- Carver, further down)
#define PG_CANARY_BYTES 64
struct pagan_batch {
    std::vector<CompactJob> compact;
    int n = 0;
    int device = 0;
    uint32_t flags = 0;
    int block = 64;
    std::vector<HostJob> jobs;
    std::vector<PgDevJob> dj;
    Arena arena;
    PgDevJob *d_jobs = nullptr;
    int *d_which = nullptr;      // [n]: ring-kernel jobs first, then the ones of the HBM wavefront kernel, the striped, the tiled
    std::vector<int> which;      // (its host copy: a pg_backptr launch scans its segment of jobs)
    int n_ring = 0, n_wide = 0, n_tiled = 0;
    int n_striped = 0;           // of the n_tiled jobs (listed first among them): filled as row strips by pg_fill_pipe<true, true>
    int strip_grid = 0;          // workgroups of that launch (the strips of a job at indices of one residue mod 8, -1 padding)
    int strip_grid_big = 0;      // ... of the launch for the jobs whose model table does not fit LDS (listed behind the others' in d_swhich)
    int *d_swhich = nullptr;     // [strip_grid] strip -> its PgDevJob (behind the n jobs of the batch) or -1
    size_t sfollow_begin = 0, sfollow_bytes = 0;     // the strips' follow words (zeroed before every launch)
    bool strips_spread = true;   // a job's strips on any XCD (PAGAN_DP_STRIP_SPREAD=0: on one, round 4's placement, checked by the feeders)
    bool strips_alone = false;   // the re-run after a strip found the strip above on another XCD: the strips' launch with nothing beside it
    int *d_tiles = nullptr;      // dp_tiles.hip: {job, tile row, tile column, position of the tile above} of all tiled jobs, ordered by
                                 // row + column; then the positions of the tiles to the left; then tile_off (pg_fill_tiles_flow)
    int *d_flow = nullptr;       // pg_fill_tiles_flow's queue head, finished tiles per diagonal, done flags (zeroed per launch)
    size_t flow_ints = 0;
    bool tiles_nolag = false;    // PAGAN_DP_TILES=nolag: tiles wait for their neighbours to finish (A/B switch)
    bool tiles_water = false;    // some job's tiles are no staircase: a tile also waits for all diagonals <= its own - 2
    bool tiles_flow = true;      // one persistent launch (default) or one launch per tile anti-diagonal (PAGAN_DP_TILES=launches)
    std::vector<int> tile_off;   // first tile of tile anti-diagonal t (tile_off.back() = total)
    GpuObjs o;                   // streams and events, from the pool and back to it (o.stream: the batch's; o.ev: around fill and traceback)
    bool forked = false;         // the tile launches and the strips on o.stream2 (between o.ev_fork and o.ev_join): the batch also has jobs of the other kernels
    int n_ring_small = 0;        // ring jobs whose model table fits the LDS cache (listed first)
    bool use_pipe = true;        // LDS-staged jobs run pg_fill_pipe (default) or the older pg_fill_ring
    int bp_pass = 1;             // pg_fill_pipe's jobs: 1 back-pointers by pg_backptr after the fill (its hot loop stores scores only),
                                 // 2 (PAGAN_DP_BP=verify, diagnostic builds that still write them in the fill) pg_backptr compares
    int max_bound = 0;           // largest traceback boundary count of any job
    int max_entries = 0;         // most traceback table entries of any job (tb[n_bound + 1])
    size_t follow_begin = 0, follow_bytes = 0;     // PgDevJob::follow / bp_done of the banded jobs, one block zeroed per launch
    // PAGAN_DP_CANARY=1: guard words behind every region of the arena (Carver)
    std::vector<size_t> guards;
    size_t *d_guards = nullptr;
    int *d_canary = nullptr;                     // [0] guards found changed by the last run, [1] the first of them
    bool strip_xcd_failure = false;              // pagan_batch_fetch: a strip found the strip above on another XCD in the launch of the strips alone, too
    unsigned canary_word = 0;                    // (PAGAN_DP_CANARY=0x...: another pattern -- what a read past a region's end then sees)
    // per-kernel brackets inside the fill (pagan_batch_last_ms_detail): 0/1 around the banded kernel, 2 behind pg_backptr,
    // 3/4 around the tiled kernel (on its own stream when the batch also has banded jobs), 5 behind the HBM wavefront
    // (o.evk; 6: behind the tiled jobs' pg_backptr)
    bool evk_set[7] = {false, false, false, false, false, false, false};
    int64_t cells = 0;
    size_t out_begin = 0;        // arena offset where the output arrays start
    bool ran = false;
    int max_path = 0;            // longest possible path of any job (Lx + Ly): pg_trace_check's grid
    bool no_follow = false;      // the re-run after a failed path check: every back-pointer by pg_backptr
    int reruns = 0;              // how often pagan_batch_fetch ran the batch again (pagan_batch_debug_reruns)
    int poke[6] = {-1, 0, 0, 0, 0, 0};     // test hook: {job, i, j, state, word, _}, applied once between fill and traceback
    // D2H staging (pinned)
    std::vector<size_t> trace_off;   // byte offsets of trace/endcell/endscore inside the arena
    std::vector<size_t> end_off, score_off;
};

namespace {

// Bump allocator over the arena: first pass sizes it, second pass hands out pointers.
// PAGAN_DP_CANARY=1 (debug): PG_CANARY_BYTES of a known pattern behind EVERY region of the arena, written before each run's
// kernels and checked after them (pg_canary, below): a store past the end of a region -- by any kernel of the batch -- turns
// up as an error of the run instead of as another region's corrupted content (or, at the arena's end, as a memory fault).
struct Carver {
    size_t cur = 0;
    char *base = nullptr;
    std::vector<size_t> *guards = nullptr;       // (canary mode) offsets of the guard words, in carving order
    template <class T> T *take(size_t count) {
        size_t off = cur;
        cur = up256(cur + sizeof(T) * (count ? count : 1));
        if (guards) { guards->push_back(cur); cur = up256(cur + PG_CANARY_BYTES); }
        return base ? reinterpret_cast<T *>(base + off) : reinterpret_cast<T *>(off);
    }
};
// check == nullptr: writes the pattern; otherwise counts the guards that no longer hold it (and names the first one)
__global__ void pg_canary(char *base, const size_t *offs, int n, int *check, unsigned word) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n) return;
    unsigned *w = reinterpret_cast<unsigned *>(base + offs[g]);
    if (!check) { for (int k = 0; k < PG_CANARY_BYTES / 4; ++k) w[k] = word; return; }
    bool bad = false;
    for (int k = 0; k < PG_CANARY_BYTES / 4; ++k) bad = bad || w[k] != word;
    if (bad) { atomicAdd(check, 1); atomicMin(check + 1, g); }
}

// Lays one job out in the arena.  With `base == nullptr` only sizes are accumulated.
void carve_job(Carver &c, const pagan_job &jb, const HostJob &hj, PgDevJob *d) {
    const pagan_graph *L = jb.left, *R = jb.right;
    const int nbL = L->bwd_off[L->n_sites], nbR = R->bwd_off[R->n_sites];
    d->Lx = hj.Lx; d->Ly = hj.Ly; d->nd = hj.Lx + hj.Ly - 1; d->S = jb.model->n_states;
    d->go = jb.model->log_gap_open; d->ge = jb.model->log_gap_ext;
    d->gE = jb.model->log_gap_end_ext; d->ng = jb.model->log_non_gap;
    d->stL = c.take<int>(L->n_sites); d->offL = c.take<int>(L->n_sites + 1);
    d->srcL = c.take<int>(nbL); d->lwL = c.take<float>(nbL);
    d->stR = c.take<int>(R->n_sites); d->offR = c.take<int>(R->n_sites + 1);
    d->srcR = c.take<int>(nbR); d->lwR = c.take<float>(nbR);
    d->table = c.take<float>((size_t)d->S * d->S);
    d->imin = c.take<int>(d->nd); d->imax = c.take<int>(d->nd); d->doff = c.take<long long>(d->nd);
    d->dsc = c.take<int>(4 * (size_t)d->nd);
    d->psc = hj.cls.empty() ? nullptr : c.take<int>(8 * ((size_t)d->nd + 1));     // one entry of padding
    d->sched = hj.cls.empty() ? nullptr : c.take<int>(hj.sched.size());
    d->hfL = hj.hfL.empty() ? nullptr : c.take<unsigned char>(hj.hfL.size());
    d->hfR = hj.hfR.empty() ? nullptr : c.take<unsigned char>(hj.hfR.size());
    d->fill_status = c.take<int>(1);
    d->cells = hj.dx.cells;
    d->n_bound = hj.n_bound;
    d->tb = c.take<int>(hj.tb.size());
}
void carve_outputs(Carver &c, const HostJob &hj, PgDevJob *d) {
    d->sc = c.take<double>(3 * (size_t)hj.dx.cells);
    d->bp = c.take<unsigned>(3 * (size_t)hj.dx.cells);
    d->trace = c.take<int>(3 * (size_t)(hj.Lx + hj.Ly));
    d->ttab = c.take<int>(8 * (size_t)hj.tb.back());
    d->segs = c.take<int>(6 * (size_t)(2 * hj.n_bound + 8));
}
// max_end of every job of the batch in one block, 64 B per job (endcell[8] at +0, endscore at +32): one copy
// brings all of them back (cfg5: 511 node alignments per walk)
constexpr size_t kEndStride = 64;
void carve_ends(Carver &c, int n, PgDevJob *dj) {
    char *ends = c.take<char>(kEndStride * (size_t)n);
    for (int k = 0; k < n; ++k) {
        dj[k].endcell = reinterpret_cast<int *>(ends + kEndStride * (size_t)k);
        dj[k].endscore = reinterpret_cast<double *>(ends + kEndStride * (size_t)k + 32);
    }
}

// PgDevJob::follow and bp_done of every job of the banded kernel, in one block (zeroed before every launch)
void carve_follow(Carver &c, int n, const std::vector<HostJob> &jobs, PgDevJob *dj, size_t *begin, size_t *bytes) {
    *begin = (c.cur + 255) & ~(size_t)255;
    c.cur = *begin;
    for (int k = 0; k < n; ++k) {
        dj[k].follow = nullptr; dj[k].bp_done = nullptr;
        if (jobs[k].cls.empty()) continue;
        dj[k].follow = c.take<int>(4);
        dj[k].bp_done = c.take<unsigned char>((((size_t)dj[k].nd + PG_FOLLOW_CHUNK - 1) / PG_FOLLOW_CHUNK + 15) & ~(size_t)15);
    }
    *bytes = c.cur - *begin;
}

// Host staging buffers are reused across batches: a level's upload is hundreds of MB, and fresh zeroed pages
// for it every time cost more than filling them (46 -> 20 ms for the 244 MB of cfg4's leaf level).
struct StagePool {
    std::mutex m;
    std::vector<std::pair<char *, size_t>> idle;
    char *take(size_t n, size_t *cap) {
        {
            std::lock_guard<std::mutex> g(m);
            for (size_t k = 0; k < idle.size(); ++k)
                if (idle[k].second >= n) {
                    char *p = idle[k].first; *cap = idle[k].second;
                    idle.erase(idle.begin() + k);
                    return p;
                }
            if (idle.size() >= 4) { std::free(idle.front().first); idle.erase(idle.begin()); }
        }
        *cap = n + n / 8 + 4096;
        return (char *)std::malloc(*cap);
    }
    void give(char *p, size_t cap) {
        if (!p) return;
        std::lock_guard<std::mutex> g(m);
        idle.emplace_back(p, cap);
    }
};
StagePool stage_pool;
struct Stage {
    char *p = nullptr;
    size_t cap = 0;
    explicit Stage(size_t n) { p = stage_pool.take(n, &cap); }
    ~Stage() { stage_pool.give(p, cap); }
    Stage(const Stage &) = delete;
    Stage &operator=(const Stage &) = delete;
    char *data() { return p; }
};

template <class T> void put(Stage &stage, const void *devptr_as_off, const T *src, size_t count) {
    if (count) std::memcpy(stage.data() + reinterpret_cast<size_t>(devptr_as_off), src, sizeof(T) * count);
}

// diagonals per workgroup of pg_backptr: PG_BP_DIAGS, halved until the grid has a few thousand workgroups (or 4 are left:
// one per wave)
static int bp_diags_per_block(int max_nd, int other_dims) {
    int dpb = PG_BP_DIAGS;
    while (dpb > 4 && (long long)((max_nd + dpb - 1) / dpb) * other_dims < 4096) dpb /= 2;
    return dpb;
}

// When a tile of pg_fill_tiles_flow may start, for a batch of n_tiles tiles on n_diag tile anti-diagonals and a
// chip of n_cu compute units.  Tiles that are no staircase need the watermark.  Otherwise a tile runs 80 steps behind its
// neighbours, except at both ends of tiles per anti-diagonal : compute units:
//   more than 1.75 x  the compute units are the bound either way, and the lag's progress flags and block-wise halo cost 15 %
//                     (measured on cfg5: 575 tiles per diagonal 65 -> 56 ms without the lag, 320 per diagonal 46 -> 48 ms);
//   fewer than 0.5 x  the chain of tile anti-diagonals is the bound (the top of a deep tree): blocks of 8 steps, 72 steps behind
//                     for twice the flags (cfg5 -3 %).
static PgTileSchedule tile_schedule(int n_tiles, int n_diag, int n_cu, bool tiles_water, bool tiles_nolag) {
    if (tiles_water) return PG_TILES_WATERMARK;
    if (4ll * n_tiles >= 7ll * n_cu * n_diag || tiles_nolag) return PG_TILES_NOLAG;
    return 2ll * n_tiles < (long long)n_cu * n_diag ? PG_TILES_LAG8 : PG_TILES_LAG16;
}

// The strips' launch (one workgroup per strip): the jobs whose model table fits LDS, then the others'
int launch_strips(pagan_batch *b, hipStream_t st, unsigned flags) {
    HIP_TRY(hipMemsetAsync(b->arena.dev + b->sfollow_begin, 0, b->sfollow_bytes, st));
    if (b->strip_grid > 0)
        hipLaunchKernelGGL((pg_fill_pipe<true, true>), dim3(b->strip_grid), dim3(pg_pipe_block()), 0, st,
                           b->d_jobs, b->d_swhich, flags, b->strip_grid);
    if (b->strip_grid_big > 0)
        hipLaunchKernelGGL((pg_fill_pipe<false, true>), dim3(b->strip_grid_big), dim3(pg_pipe_block()), 0, st,
                           b->d_jobs, b->d_swhich + b->strip_grid, flags, b->strip_grid_big);
    return PAGAN_OK;
}

// The stream of the tile launches and the strips: the second one, behind what the batch's stream holds so far, when the batch
// also has jobs of the other kernels
int fork_tile_stream(pagan_batch *b, hipStream_t *st) {
    *st = b->o.stream;
    if (b->forked) {
        HIP_TRY(hipEventRecord(b->o.ev_fork, b->o.stream));
        HIP_TRY(hipStreamWaitEvent(b->o.stream2, b->o.ev_fork, 0));
        *st = b->o.stream2;
    }
    return PAGAN_OK;
}

// pg_backptr over the jobs which[first .. first + count) of the batch
void launch_backptr(pagan_batch *b, hipStream_t st, int first, int count, unsigned flags) {
    int max_nd = 1, max_w = 1;
    for (int q = first; q < first + count; ++q) { const int k = b->which[q]; max_nd = std::max(max_nd, b->dj[k].nd); max_w = std::max(max_w, b->jobs[k].dx.max_width); }
    const int zc = (max_w + PG_BP_CELLS - 1) / PG_BP_CELLS, dpb = bp_diags_per_block(max_nd, count * zc);
    hipLaunchKernelGGL(pg_backptr, dim3((max_nd + dpb - 1) / dpb, count, zc), dim3(256), 0, st, b->d_jobs, b->d_which + first, flags, dpb);
}

int launch_fill(pagan_batch *b, const DpSwitches &sw) {
    // Full-matrix score check (PG_FLAG_SCORE_CHECK; dp_kernels.hip, pg_backptr): whoever writes a cell's back-pointers has just
    // re-evaluated its three scores from the stored scores of its predecessors -- comparing them with the cell's own stored
    // scores proves the recurrence at every cell.  On for the banded kernel's jobs (the follower workgroups do it on compute
    // units the fill leaves idle) and for batches with row strips (scores cross workgroups on a landing rule there);
    // PAGAN_DP_SCORE_CHECK=0 switches it off, =all extends it to every tiled job's pass.
    unsigned chk_banded = PG_FLAG_SCORE_CHECK, chk_wide = b->n_striped > 0 ? PG_FLAG_SCORE_CHECK : 0u;
    if (sw.score_check == DpSwitches::CHECK_OFF) { chk_banded = 0; chk_wide = 0; }
    else if (sw.score_check == DpSwitches::CHECK_ALL) chk_wide = PG_FLAG_SCORE_CHECK;
    const unsigned spread = b->strips_spread ? PG_FLAG_STRIPS_SPREAD : 0u;
    hipStream_t tile_stream = nullptr;
    static std::atomic<int> n_cu_dev[64];
    bool ev3_recorded = false;
    if (b->n_striped > 0 && b->strips_alone) {
        // (workgroup g of a dispatch runs on XCD g % 8 -- what puts a job's strips on one XCD -- when nothing else is being
        //  dispatched beside it: first on the batch's stream, everything else behind it)
        if (const int rc = launch_strips(b, b->o.stream, ((b->flags & 0x400u) ? b->flags : (b->flags & ~0x800u)) | spread)) return rc;
    }
    if (b->n_striped > 0 && b->tile_off.size() <= 1) {
        // (the strips' stream: beside the banded kernels, as the tiles')
        if (const int rc = fork_tile_stream(b, &tile_stream)) return rc;
    }
    if (b->tile_off.size() > 1) {
        static std::atomic<bool> tiles_set_dev[64];
        std::atomic<bool> &tiles_set = tiles_set_dev[b->device & 63];
        if (!tiles_set.load()) {
            HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(pg_fill_tiles),
                                        hipFuncAttributeMaxDynamicSharedMemorySize, (int)pg_tiles_lds_bytes()));
            HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(pg_fill_tiles_flow),
                                        hipFuncAttributeMaxDynamicSharedMemorySize, (int)pg_tiles_lds_bytes()));
            int n_cu = 0;
            HIP_TRY(hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, b->device));
            n_cu_dev[b->device & 63].store(n_cu > 0 ? n_cu : 256);
            tiles_set.store(true);
        }
        // one launch per tile anti-diagonal, all tiled jobs of the batch together; beside the other kernels
        if (const int rc = fork_tile_stream(b, &tile_stream)) return rc;
    }
    if (b->n_ring > 0) {
        // > 64 KB of dynamic LDS has to be opted into once per device (a process may drive several)
        static std::atomic<bool> lds_set_dev[64];
        std::atomic<bool> &lds_set = lds_set_dev[b->device & 63];
        if (!lds_set.load()) {
            HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(pg_fill_ring<true>),
                                        hipFuncAttributeMaxDynamicSharedMemorySize, (int)pg_ring_lds_bytes()));
            HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(pg_fill_ring<false>),
                                        hipFuncAttributeMaxDynamicSharedMemorySize, (int)pg_ring_lds_bytes()));
            lds_set.store(true);
        }
        // model tables of <= 16 states (DNA: 15) are cached in LDS; larger ones stay in HBM/L2
        const int n_small = b->n_ring_small, n_big = b->n_ring - b->n_ring_small;
        HIP_TRY(hipEventRecord(b->o.evk[0], b->o.stream)); b->evk_set[0] = true;
        if (b->use_pipe) {
            // Follower workgroups behind the fill's (dp_pipe.hip, pipe_follower): they write the back-pointers of the diagonals
            // whose scores have landed while the fill goes on, on compute units the banded fill leaves idle.  Workgroup g of
            // a dispatch runs on XCD g % 8 and a follower serves the fill workgroups of its own XCD (it shares their L2), so
            // eight followers per round of eight jobs are the unit; what they do not get to is left to pg_backptr below.
            const bool follow = b->bp_pass == 1 && b->follow_bytes > 0 && !b->no_follow && sw.follow;      // (PAGAN_DP_FOLLOW=0)
            if (b->follow_bytes > 0) HIP_TRY(hipMemsetAsync(b->arena.dev + b->follow_begin, 0, b->follow_bytes, b->o.stream));
            // (a dispatch of more than 32 jobs fills the chip by itself: pg_backptr afterwards, on every unit, is the faster pass)
            auto followers = [&](int n_fill) { return follow && n_fill <= 32 ? std::min(96, 48 * ((n_fill + 7) / 8)) : 0; };
            if (n_small > 0)
                hipLaunchKernelGGL((pg_fill_pipe<true, false>), dim3(n_small + followers(n_small)), dim3(pg_pipe_block()), 0 /* its LDS is static */, b->o.stream,
                                   b->d_jobs, b->d_which, b->flags | chk_banded, n_small);
            if (n_big > 0)
                hipLaunchKernelGGL((pg_fill_pipe<false, false>), dim3(n_big + followers(n_big)), dim3(pg_pipe_block()), 0, b->o.stream,
                                   b->d_jobs, b->d_which + n_small, b->flags | chk_banded, n_big);
            HIP_TRY(hipEventRecord(b->o.evk[1], b->o.stream)); b->evk_set[1] = true;
            if (b->bp_pass) {
                launch_backptr(b, b->o.stream, 0, b->n_ring, (b->flags & 0xffu) | (b->bp_pass == 2 ? 0x100u : chk_banded));
                HIP_TRY(hipEventRecord(b->o.evk[2], b->o.stream)); b->evk_set[2] = true;
            }
        } else {
            b->evk_set[1] = false;
            if (n_small > 0)
                hipLaunchKernelGGL(pg_fill_ring<true>, dim3(n_small), dim3(576), pg_ring_lds_bytes(), b->o.stream,
                                   b->d_jobs, b->d_which, b->flags);
            if (n_big > 0)
                hipLaunchKernelGGL(pg_fill_ring<false>, dim3(n_big), dim3(576), pg_ring_lds_bytes(), b->o.stream,
                                   b->d_jobs, b->d_which + n_small, b->flags);
        }
    }
    if (b->n_wide > 0) {
        dim3 grid(b->n_wide);
        const int *which = b->d_which + b->n_ring;
        switch (b->block) {
        case 64: hipLaunchKernelGGL(pg_fill_wavefront<64>, grid, dim3(64), 0, b->o.stream, b->d_jobs, which, b->flags); break;
        case 256: hipLaunchKernelGGL(pg_fill_wavefront<256>, grid, dim3(256), 0, b->o.stream, b->d_jobs, which, b->flags); break;
        default: hipLaunchKernelGGL(pg_fill_wavefront<1024>, grid, dim3(1024), 0, b->o.stream, b->d_jobs, which, b->flags); break;
        }
        HIP_TRY(hipEventRecord(b->o.evk[5], b->o.stream)); b->evk_set[5] = true;
    }
    if (b->n_striped > 0 && !b->strips_alone) {
        // row strips of the wide jobs on the banded kernel: one workgroup per strip, a job's strips on one XCD
        HIP_TRY(hipEventRecord(b->o.evk[3], tile_stream)); b->evk_set[3] = true; ev3_recorded = true;
        if (const int rc = launch_strips(b, tile_stream, b->flags | spread)) return rc;
    }
    if (b->tile_off.size() > 1) {
        // after the banded kernels: their workgroups get compute units first; the persistent waves below hold theirs
        hipStream_t st = tile_stream;
        if (!ev3_recorded) { HIP_TRY(hipEventRecord(b->o.evk[3], st)); b->evk_set[3] = true; }
        if (b->tiles_flow) {
            // one persistent wave per compute unit (a tile fills the LDS) drains the batch's tiles in dependency order
            const int n_tiles = b->tile_off.back(), n_diag = (int)b->tile_off.size() - 1;
            // no more waves than can have a tile to work on: the tiles of two anti-diagonals (a tile runs 80 steps behind
            // its neighbours) -- a persistent wave holds its compute unit's LDS, which the batch's banded jobs need too
            int widest = 1;
            for (int t = 0; t < n_diag; ++t) widest = std::max(widest, b->tile_off[t + 1] - b->tile_off[t]);
            const int n_cu = n_cu_dev[b->device & 63].load();
            const int waves = std::min({n_tiles, n_cu, 2 * widest + 8});
            HIP_TRY(hipMemsetAsync(b->d_flow, 0, sizeof(int) * b->flow_ints, st));
            hipLaunchKernelGGL(pg_fill_tiles_flow, dim3(waves), dim3(64), pg_tiles_lds_bytes(),
                               st, b->d_jobs, b->d_tiles, n_tiles, n_diag, b->d_flow, b->flags,
                               (int)tile_schedule(n_tiles, n_diag, n_cu, b->tiles_water, b->tiles_nolag));
        } else {
            for (size_t t = 0; t + 1 < b->tile_off.size(); ++t) {
                const int cnt = b->tile_off[t + 1] - b->tile_off[t];
                if (cnt > 0)
                    hipLaunchKernelGGL(pg_fill_tiles, dim3(cnt), dim3(64), pg_tiles_lds_bytes(), st, b->d_jobs,
                                       b->d_tiles + 4 * (size_t)b->tile_off[t], b->flags);
            }
        }
    }
    if (b->tile_off.size() > 1 || b->n_striped > 0) {
        HIP_TRY(hipEventRecord(b->o.evk[4], tile_stream)); b->evk_set[4] = true;
        // the tiled fill (and the strips) store scores only: their jobs' back-pointers by the pass, behind them on the same stream
        if (b->n_tiled > 0) {
            launch_backptr(b, tile_stream, b->n_ring + b->n_wide, b->n_tiled, (b->flags & 0xffu) | chk_wide);
            HIP_TRY(hipEventRecord(b->o.evk[6], tile_stream)); b->evk_set[6] = true;
        }
    }
    if ((b->tile_off.size() > 1 || b->n_striped > 0) && b->forked) {
        HIP_TRY(hipEventRecord(b->o.ev_join, b->o.stream2));
        HIP_TRY(hipStreamWaitEvent(b->o.stream, b->o.ev_join, 0));
    }
    HIP_TRY(hipGetLastError());
    return PAGAN_OK;
}

// ---- pagan_batch_create's stages ------------------------------------------------------------------------------------
// compact -> plan and route -> group -> build_tile_list / order_strips (dp_plan.cpp) -> carve -> stage -> rebase -> device objects

// dead sites out (see CompactJob): the stages behind this one work on the effective jobs
void compact_jobs(pagan_batch *b, const pagan_job *jobs, bool allow, std::vector<pagan_job> *eff) {
    b->compact.resize(b->n);
    parallel_jobs(b->n, [&](int k) { compact_job(jobs[k], allow, &b->compact[k], &(*eff)[k]); });
}

int plan_jobs(pagan_batch *b, const std::vector<pagan_job> &eff, const DpSwitches &sw, bool allow_strips) {
    const int n = b->n;
    std::vector<int> job_rc(n, PAGAN_OK);
    // a level of few alignments: the threads the jobs leave idle go into each job's own plan
    const int hw = (int)std::thread::hardware_concurrency();
    const int inner = std::max(1, std::min(8, (hw > 0 ? std::min(hw, 16) : 1) / std::max(n, 1)));
    parallel_jobs(n, [&](int k) { job_rc[k] = validate_job(eff[k], &b->jobs[k], sw, allow_strips, inner); });
    for (int k = 0; k < n; ++k) if (job_rc[k] != PAGAN_OK) return job_rc[k];
    return PAGAN_OK;
}

// The jobs by route, and what the launches need to know about all of them.  b->which: small-table banded, big-table banded,
// wavefront, striped, tiled (striped and tiled jobs: one back-pointer pass behind both fills; the tiled fill reaches its jobs
// through the tile list, pg_backptr through this).
struct Groups { std::vector<int> by_route[5]; };
void group_jobs(pagan_batch *b, Groups *g) {
    int max_w = 0;
    for (int k = 0; k < b->n; ++k) {
        const HostJob &hj = b->jobs[k];
        b->cells += b->compact[k].on ? b->compact[k].cells0 : hj.dx.cells;       // the caller's cells
        if (hj.n_bound > b->max_bound) b->max_bound = hj.n_bound;
        b->max_path = std::max(b->max_path, hj.Lx + hj.Ly);
        if (hj.n_bound > 0 && hj.tb[hj.n_bound + 1] > b->max_entries) b->max_entries = hj.tb[hj.n_bound + 1];
        g->by_route[hj.route].push_back(k);
        if (hj.route == WAVEFRONT && hj.dx.max_width > max_w) max_w = hj.dx.max_width;
    }
    for (Route r : {PIPE_SMALL, PIPE_BIG, WAVEFRONT, STRIPS, TILES}) b->which.insert(b->which.end(), g->by_route[r].begin(), g->by_route[r].end());
    b->n_ring_small = (int)g->by_route[PIPE_SMALL].size();
    b->n_ring = b->n_ring_small + (int)g->by_route[PIPE_BIG].size();
    b->n_wide = (int)g->by_route[WAVEFRONT].size();
    b->n_striped = (int)g->by_route[STRIPS].size();
    b->n_tiled = b->n_striped + (int)g->by_route[TILES].size();
    b->block = max_w <= 64 ? 64 : (max_w <= 512 ? 256 : 1024);
}

// A strip's own regions of the arena (it shares everything else with its job)
struct StripDev { int job, q; int *psc, *sched, *follow; };
// The batch's own arrays in the arena
struct BatchRegions { PgDevJob *jobs; int *which, *swhich, *tiles, *flow; size_t in_bytes; };

// Sizes and offsets (`c` has no base): inputs first (one contiguous upload), outputs after.
BatchRegions carve_batch(Carver &c, pagan_batch *b, const std::vector<pagan_job> &eff, std::vector<StripDev> *sdev, size_t n_swhich, size_t n_tile_ints) {
    const int n = b->n;
    BatchRegions r;
    r.jobs = c.take<PgDevJob>((size_t)n + sdev->size());
    r.which = c.take<int>(n);
    r.swhich = c.take<int>(n_swhich);
    for (StripDev &sd : *sdev) {
        const StripPlan &sp = b->jobs[sd.job].strips[sd.q];
        sd.psc = c.take<int>(sp.psc.size()); sd.sched = c.take<int>(sp.sched.size());
    }
    r.tiles = c.take<int>(n_tile_ints);
    r.flow = c.take<int>(b->flow_ints);
    for (int k = 0; k < n; ++k) carve_job(c, eff[k], b->jobs[k], &b->dj[k]);
    r.in_bytes = c.cur;
    b->out_begin = r.in_bytes;
    for (int k = 0; k < n; ++k) carve_outputs(c, b->jobs[k], &b->dj[k]);
    carve_ends(c, n, b->dj.data());
    carve_follow(c, n, b->jobs, b->dj.data(), &b->follow_begin, &b->follow_bytes);
    b->sfollow_begin = c.cur;
    for (StripDev &sd : *sdev) sd.follow = c.take<int>(4);
    b->sfollow_bytes = c.cur - b->sfollow_begin;
    b->arena.size = c.cur;
    return r;
}

int take_arena(pagan_batch *b) {
    b->arena.dev = slab_alloc(arena_pool, b->device, b->arena.size, &b->arena.cap);
    if (!b->arena.dev) {
        drain_slabs(arena_pool, b->device);              // the idle arenas may be what is in the way -- and the other pools' (parent
        pagan::parent_release_cache();                   // builder slabs, forward/backward arenas: round 4 advisor)
        pagan_fb_internal_release_cache();
        HIP_TRY(hipMalloc((void **)&b->arena.dev, b->arena.size));
    }
    if (!b->guards.empty()) {
        // (the follow words are zeroed in one sweep per run, guards and all: those regions go unguarded)
        auto zeroed = [&](size_t o) { return (o >= b->follow_begin && o < b->follow_begin + b->follow_bytes) || (o >= b->sfollow_begin && o < b->sfollow_begin + b->sfollow_bytes); };
        b->guards.erase(std::remove_if(b->guards.begin(), b->guards.end(), zeroed), b->guards.end());
        HIP_TRY(hipMalloc((void **)&b->d_guards, b->guards.size() * sizeof(size_t)));
        HIP_TRY(hipMalloc((void **)&b->d_canary, 2 * sizeof(int)));
        HIP_TRY(hipMemcpy(b->d_guards, b->guards.data(), b->guards.size() * sizeof(size_t), hipMemcpyHostToDevice));
    }
    return PAGAN_OK;
}

// The jobs' inputs and the strips' into the staging buffer (the offsets of carve_batch index it)
void stage_inputs(Stage &stage, const pagan_batch *b, const std::vector<pagan_job> &eff, const std::vector<StripDev> &sdev, const DpSwitches &sw) {
    parallel_jobs(b->n, [&](int k) {
        const pagan_job &jb = eff[k];
        const HostJob &hj = b->jobs[k];
        const PgDevJob &d = b->dj[k];
        const pagan_graph *L = jb.left, *R = jb.right;
        put(stage, d.stL, L->state, L->n_sites); put(stage, d.offL, L->bwd_off, L->n_sites + 1);
        put(stage, d.srcL, L->bwd_src, L->bwd_off[L->n_sites]); put(stage, d.lwL, L->bwd_logw, L->bwd_off[L->n_sites]);
        put(stage, d.stR, R->state, R->n_sites); put(stage, d.offR, R->bwd_off, R->n_sites + 1);
        put(stage, d.srcR, R->bwd_src, R->bwd_off[R->n_sites]); put(stage, d.lwR, R->bwd_logw, R->bwd_off[R->n_sites]);
        put(stage, d.table, jb.model->log_score, (size_t)d.S * d.S);
        put(stage, d.imin, hj.dx.imin.data(), hj.dx.imin.size());
        put(stage, d.imax, hj.dx.imax.data(), hj.dx.imax.size());
        put(stage, d.doff, hj.dx.doff.data(), hj.dx.doff.size());
        {
            int *packed = reinterpret_cast<int *>(stage.data() + reinterpret_cast<size_t>(d.dsc));     // written in place
            for (size_t t = 0; t < hj.dx.imin.size(); ++t) {
                packed[4 * t] = hj.dx.imin[t]; packed[4 * t + 1] = hj.dx.imax[t];
                packed[4 * t + 2] = (int)(hj.dx.doff[t] & 0xffffffffLL); packed[4 * t + 3] = (int)(hj.dx.doff[t] >> 32);
            }
        }
        if (!hj.cls.empty()) {
            pack_pipe_descriptors(hj, d.S, sw, reinterpret_cast<int *>(stage.data() + reinterpret_cast<size_t>(d.psc)));
            put(stage, d.sched, hj.sched.data(), hj.sched.size());
            if (d.hfL) { put(stage, d.hfL, hj.hfL.data(), hj.hfL.size()); put(stage, d.hfR, hj.hfR.data(), hj.hfR.size()); }
        }
        put(stage, d.tb, hj.tb.data(), hj.tb.size());
        const int zero = 0;
        put(stage, d.fill_status, &zero, 1);          // the staging buffer is reused, not zeroed
    });
    parallel_jobs((int)sdev.size(), [&](int g) {
        const StripPlan &sp = b->jobs[sdev[g].job].strips[sdev[g].q];
        put(stage, sdev[g].psc, sp.psc.data(), sp.psc.size());
        put(stage, sdev[g].sched, sp.sched.data(), sp.sched.size());
    });
}

// Offsets -> device pointers: the jobs', the strips' device jobs behind them, the batch's own arrays
void rebase_batch(pagan_batch *b, const std::vector<StripDev> &sdev, const BatchRegions &r) {
    const int n = b->n;
    b->trace_off.resize(n); b->end_off.resize(n); b->score_off.resize(n);
    char *base = b->arena.dev;
    auto rebase = [&](auto *&p) { p = reinterpret_cast<std::remove_reference_t<decltype(p)>>(base + reinterpret_cast<size_t>(p)); };
    for (int k = 0; k < n; ++k) {
        PgDevJob &d = b->dj[k];
        b->trace_off[k] = reinterpret_cast<size_t>(d.trace);
        b->end_off[k] = reinterpret_cast<size_t>(d.endcell);
        b->score_off[k] = reinterpret_cast<size_t>(d.endscore);
        rebase(d.stL); rebase(d.offL); rebase(d.srcL); rebase(d.lwL);
        rebase(d.stR); rebase(d.offR); rebase(d.srcR); rebase(d.lwR);
        rebase(d.table); rebase(d.imin); rebase(d.imax); rebase(d.doff); rebase(d.tb); rebase(d.dsc); if (d.psc) { rebase(d.psc); rebase(d.sched); } if (d.hfL) { rebase(d.hfL); rebase(d.hfR); } rebase(d.fill_status);
        rebase(d.sc); rebase(d.bp);
        rebase(d.trace); rebase(d.endcell); rebase(d.endscore); rebase(d.segs); rebase(d.ttab);
        if (d.follow) { rebase(d.follow); rebase(d.bp_done); }
    }
    for (size_t g = 0; g < sdev.size(); ++g) {
        // a strip: the parent's job with its own descriptors (the pointer moved back so that psc[d] works from d_first on),
        // schedule and follow words
        const StripPlan &sp = b->jobs[sdev[g].job].strips[sdev[g].q];
        PgDevJob d = b->dj[sdev[g].job];
        d.psc = reinterpret_cast<int *>(base + reinterpret_cast<size_t>(sdev[g].psc)) - 8 * (ptrdiff_t)sp.d0;
        d.sched = reinterpret_cast<int *>(base + reinterpret_cast<size_t>(sdev[g].sched));
        d.follow = reinterpret_cast<int *>(base + reinterpret_cast<size_t>(sdev[g].follow));
        d.bp_done = nullptr;
        d.nd = sp.d1;
        d.is_strip = 1; d.strip_row0 = sp.r0; d.d_first = sp.d0; d.feed_wave = sp.feed_wave; d.col_first = sp.col_first;
        d.pdsc = b->dj[sdev[g].job].dsc;
        d.prev_follow = nullptr; d.prev_nd = 0;
        if (sdev[g].q > 0) {                                      // (the strip above is the entry before: a job's strips are listed in order)
            d.prev_follow = b->dj[(size_t)n + g - 1].follow;
            d.prev_nd = b->dj[(size_t)n + g - 1].nd;
        }
        b->dj[(size_t)n + g] = d;
    }
    b->d_swhich = reinterpret_cast<int *>(base + reinterpret_cast<size_t>(r.swhich));
    b->d_jobs = reinterpret_cast<PgDevJob *>(base + reinterpret_cast<size_t>(r.jobs));
    b->d_which = reinterpret_cast<int *>(base + reinterpret_cast<size_t>(r.which));
    b->d_tiles = reinterpret_cast<int *>(base + reinterpret_cast<size_t>(r.tiles));
    b->d_flow = reinterpret_cast<int *>(base + reinterpret_cast<size_t>(r.flow));
}

// streams and events come from a per-device pool: a level of a tree walk is followed by the next, and creating and
// destroying a dozen of them per batch cost milliseconds of the walk's wall-clock
int take_gpu_objs(pagan_batch *b) {
    GpuObjs &o = b->o;
    if (!gpu_pool.take(b->device, &o)) {
        HIP_TRY(hipStreamCreate(&o.stream));
        HIP_TRY(hipStreamCreate(&o.stream2));
        for (auto &e : o.ev) HIP_TRY(hipEventCreate(&e));
        for (auto &e : o.evk) HIP_TRY(hipEventCreate(&e));
        HIP_TRY(hipEventCreateWithFlags(&o.ev_fork, hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&o.ev_join, hipEventDisableTiming));
    }
    b->forked = b->n_tiled > 0 && b->n_ring + b->n_wide > 0;
    return PAGAN_OK;
}

// pagan_batch_create; allow_strips = false: every wide job on the tiled kernel (pagan_dp_align_batch's third attempt)
int batch_create(int32_t n, const pagan_job *jobs, const pagan_opts *opts, const DpSwitches &sw, bool allow_strips, pagan_batch **out) {
    if (n <= 0 || !jobs || !out) return PAGAN_E_ARG;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return PAGAN_E_NODEVICE;
    pagan_batch *b = new (std::nothrow) pagan_batch();
    if (!b) return PAGAN_E_NOMEM;
    struct Guard { pagan_batch *b; ~Guard() { if (b) pagan_batch_destroy(b); } } guard{b};
    b->n = n;
    b->flags = opts ? opts->flags : 0;
    b->strips_spread = sw.strip_spread;
    if (opts && opts->device >= 0) HIP_TRY(hipSetDevice(opts->device));
    HIP_TRY(hipGetDevice(&b->device));
    b->jobs.resize(n);
    b->dj.resize(n);
    // A/B switch: PAGAN_DP_FILL=ring runs the barrier-per-diagonal LDS kernel instead of the register wavefront
    b->use_pipe = sw.fill != DpSwitches::FILL_RING;
    b->bp_pass = sw.bp;
    // ("fill" = the fill kernel writes its own back-pointers: true of the ring kernel only -- pg_fill_pipe's loop stores scores
    //  and nothing else, so with it the pass always runs)
    if (b->use_pipe && b->bp_pass == 0) b->bp_pass = 1;
    b->flags |= sw.debug_flags;
    auto now = [] { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    const double tc0 = now();
    std::vector<pagan_job> eff(jobs, jobs + n);
    compact_jobs(b, jobs, sw.compact, &eff);
    if (const int rc = plan_jobs(b, eff, sw, allow_strips)) return rc;
    Groups groups;
    group_jobs(b, &groups);
    std::vector<int> tile_list;
    build_tile_list(b->jobs, groups.by_route[TILES], &tile_list, &b->tile_off, &b->tiles_water);
    if (!tile_list.empty()) {
        if (sw.tiles == DpSwitches::TILES_WATERMARK) b->tiles_water = true;
        if (sw.tiles == DpSwitches::TILES_NOLAG) b->tiles_nolag = true;
        b->flow_ints = b->tile_off.size() + (size_t)b->tile_off.back() + 1;     // queue head, finished tiles per diagonal, progress per tile, give-up flag
        b->tiles_flow = sw.tiles != DpSwitches::TILES_LAUNCHES;   // A/B switch
    }
    std::vector<StripDev> sdev;
    std::vector<int> swhich;
    {
        std::vector<std::pair<int, int>> strips;
        int grid[2] = {0, 0};
        order_strips(b->jobs, eff, groups.by_route[STRIPS], n, b->strips_spread, &strips, &swhich, grid);
        b->strip_grid = grid[0]; b->strip_grid_big = grid[1];
        for (const auto &js : strips) sdev.push_back({js.first, js.second, nullptr, nullptr, nullptr});
        b->dj.resize((size_t)n + sdev.size());
    }

    const double tc1 = now();
    // pass 1: sizes
    Carver sizer;
    if (sw.canary) { sizer.guards = &b->guards; b->canary_word = sw.canary_word; }
    const BatchRegions regions = carve_batch(sizer, b, eff, &sdev, swhich.size(), tile_list.size());
    if (const int rc = take_arena(b)) return rc;
    const double tc2 = now();

    // pass 2: stage inputs (offsets from pass 1 index the staging buffer), then rebase.
    Stage stage(regions.in_bytes);
    if (!stage.data()) return PAGAN_E_NOMEM;
    stage_inputs(stage, b, eff, sdev, sw);
    const double tc3 = now();
    rebase_batch(b, sdev, regions);
    std::memcpy(stage.data() + reinterpret_cast<size_t>(regions.jobs), b->dj.data(), sizeof(PgDevJob) * b->dj.size());
    std::memcpy(stage.data() + reinterpret_cast<size_t>(regions.which), b->which.data(), sizeof(int) * n);
    if (!swhich.empty()) std::memcpy(stage.data() + reinterpret_cast<size_t>(regions.swhich), swhich.data(), sizeof(int) * swhich.size());
    if (!tile_list.empty()) std::memcpy(stage.data() + reinterpret_cast<size_t>(regions.tiles), tile_list.data(), sizeof(int) * tile_list.size());
    if (const int rc = take_gpu_objs(b)) return rc;
    HIP_TRY(hipMemcpyAsync(b->arena.dev, stage.data(), regions.in_bytes, hipMemcpyHostToDevice, b->o.stream));
    HIP_TRY(hipStreamSynchronize(b->o.stream));
    if (sw.verbose)
        std::fprintf(stderr, "pagan_dp: create: plan %.1f ms, hipMalloc of %.0f MB %.1f ms, staging %.0f MB %.1f ms, upload %.1f ms\n",
                     1e3 * (tc1 - tc0), b->arena.size / 1048576.0, 1e3 * (tc2 - tc1), regions.in_bytes / 1048576.0, 1e3 * (tc3 - tc2),
                     1e3 * (now() - tc3));
    guard.b = nullptr;
    *out = b;
    return PAGAN_OK;
}

} // namespace

extern "C" {

const char *pagan_dp_version(void) { return "pagan_dp 0.1 (gfx950 wavefront)"; }

int pagan_dp_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int pagan_dp_select_device(int32_t device) {
    HIP_TRY(hipSetDevice(device));
    return PAGAN_OK;
}

int pagan_batch_create(int32_t n, const pagan_job *jobs, const pagan_opts *opts, pagan_batch **out) {
    return batch_create(n, jobs, opts, DpSwitches::read(), true, out);
}

int pagan_batch_run(pagan_batch *b) {
    if (!b) return PAGAN_E_ARG;
    HIP_TRY(hipSetDevice(b->device));
    if (b->d_guards) {
        // (on the batch's stream, ahead of everything the run launches there; the tiled jobs' stream waits for an event of this one)
        const int init[2] = {0, 0x7fffffff};
        HIP_TRY(hipMemcpyAsync(b->d_canary, init, sizeof init, hipMemcpyHostToDevice, b->o.stream));
        hipLaunchKernelGGL(pg_canary, dim3(((int)b->guards.size() + 255) / 256), dim3(256), 0, b->o.stream, b->arena.dev, b->d_guards, (int)b->guards.size(), (int *)nullptr, b->canary_word);
    }
    HIP_TRY(hipEventRecord(b->o.ev[0], b->o.stream));
    int rc = launch_fill(b, DpSwitches::read());
    if (rc != PAGAN_OK) return rc;
    HIP_TRY(hipEventRecord(b->o.ev[1], b->o.stream));
    if (b->poke[0] >= 0 && b->poke[0] < b->n) {
        hipLaunchKernelGGL(pg_debug_poke_bp, dim3(1), dim3(64), 0, b->o.stream, b->d_jobs, b->poke[0], b->poke[1], b->poke[2], b->poke[3], (unsigned)b->poke[4]);
        b->poke[0] = -1;
    }
    {
        // (pg_fill_tiles_flow's give-up word sits behind its per-diagonal counters and per-tile flags)
        const bool flow = b->tile_off.size() > 1 && b->tiles_flow;
        const int *gave_up = flow ? b->d_flow + 1 + ((int)b->tile_off.size() - 1) + b->tile_off.back() : nullptr;
        hipLaunchKernelGGL(pg_end_corner, dim3(b->n), dim3(64), 0, b->o.stream, b->d_jobs, gave_up);
    }
    if (b->max_bound > 0 && b->max_entries > 0)
        hipLaunchKernelGGL(pg_trace_spec, dim3((b->max_entries + 127) / 128, b->n), dim3(128), 0, b->o.stream, b->d_jobs);
    hipLaunchKernelGGL(pg_trace_compose, dim3(b->n), dim3(64), 0, b->o.stream, b->d_jobs);
    if (b->max_bound > 0)
        hipLaunchKernelGGL(pg_trace_emit, dim3((2 * b->max_bound + 8 + 63) / 64, b->n), dim3(64), 0, b->o.stream, b->d_jobs);
    // every visited cell re-evaluated from the stored scores (always on: a back-pointer written from a score that had
    // not landed yet would otherwise be a valid-looking pointer to the wrong cell)
    if (b->max_path > 0)
        hipLaunchKernelGGL(pg_trace_check, dim3((b->max_path + 255) / 256, b->n), dim3(256), 0, b->o.stream, b->d_jobs, b->flags & 0xffu);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(b->o.ev[2], b->o.stream));
    if (b->d_guards)
        hipLaunchKernelGGL(pg_canary, dim3(((int)b->guards.size() + 255) / 256), dim3(256), 0, b->o.stream, b->arena.dev, b->d_guards, (int)b->guards.size(), b->d_canary, b->canary_word);
    b->ran = true;
    return PAGAN_OK;
}

// (canary mode) after the run's kernels: PAGAN_OK, or PAGAN_E_INTERNAL with the first changed guard named on stderr
static int canary_verdict(pagan_batch *b) {
    if (!b->d_guards || !b->ran) return PAGAN_OK;
    int got[2] = {0, 0};
    HIP_TRY(hipMemcpy(got, b->d_canary, sizeof got, hipMemcpyDeviceToHost));
    if (got[0] == 0) return PAGAN_OK;
    std::fprintf(stderr, "pagan_dp: CANARY: %d of %zu guard words changed during the run; the first is guard %d at arena offset %zu (arena of %zu bytes, outputs from %zu)\n",
                 got[0], b->guards.size(), got[1], b->guards[(size_t)got[1]], b->arena.size, b->out_begin);
    return PAGAN_E_INTERNAL;
}

int pagan_batch_sync(pagan_batch *b) {
    if (!b) return PAGAN_E_ARG;
    HIP_TRY(hipStreamSynchronize(b->o.stream));
    return canary_verdict(b);
}

int pagan_batch_last_ms(pagan_batch *b, double ms[2]) {
    if (!b || !b->ran) return PAGAN_E_ARG;
    HIP_TRY(hipEventSynchronize(b->o.ev[2]));
    float a = 0, c = 0;
    HIP_TRY(hipEventElapsedTime(&a, b->o.ev[0], b->o.ev[1]));
    HIP_TRY(hipEventElapsedTime(&c, b->o.ev[1], b->o.ev[2]));
    ms[0] = a; ms[1] = c;
    return PAGAN_OK;
}

// ms[0] banded fill kernel (pg_fill_pipe / pg_fill_ring), ms[1] pg_backptr, ms[2] tiled fill, ms[3] HBM wavefront fill (from
// the end of whatever ran before it on the stream), ms[4] end corner + traceback, ms[5] the whole fill; -1: not launched
int pagan_batch_last_ms_detail(pagan_batch *b, double ms[6]) {
    if (!b || !b->ran) return PAGAN_E_ARG;
    HIP_TRY(hipEventSynchronize(b->o.ev[2]));
    auto span = [&](hipEvent_t a, hipEvent_t c, bool ok) -> double {
        float t = 0;
        if (!ok || hipEventElapsedTime(&t, a, c) != hipSuccess) return -1.0;
        return t;
    };
    ms[0] = span(b->o.evk[0], b->o.evk[1], b->evk_set[0] && b->evk_set[1]);
    if (ms[0] < 0 && b->evk_set[0]) ms[0] = span(b->o.evk[0], b->o.ev[1], true);           // (the ring kernel: no pass behind it)
    ms[1] = span(b->o.evk[1], b->o.evk[2], b->evk_set[1] && b->evk_set[2]);
    {   // (+ the pass over the tiled jobs, which runs behind the tiled fill on its stream)
        const double t2 = span(b->o.evk[4], b->o.evk[6], b->evk_set[4] && b->evk_set[6]);
        if (t2 >= 0) ms[1] = (ms[1] < 0 ? 0.0 : ms[1]) + t2;
    }
    ms[2] = span(b->o.evk[3], b->o.evk[4], b->evk_set[3] && b->evk_set[4]);
    ms[3] = b->evk_set[5] ? span(b->evk_set[2] ? b->o.evk[2] : (b->evk_set[1] ? b->o.evk[1] : b->o.ev[0]), b->o.evk[5], true) : -1.0;
    ms[4] = span(b->o.ev[1], b->o.ev[2], true);
    ms[5] = span(b->o.ev[0], b->o.ev[1], true);
    return PAGAN_OK;
}

int64_t pagan_batch_cells(const pagan_batch *b) { return b ? b->cells : 0; }

int pagan_batch_fetch(pagan_batch *b, pagan_result *out) {
    if (!b || !out || !b->ran) return PAGAN_E_ARG;
    const DpSwitches sw = DpSwitches::read();
    HIP_TRY(hipStreamSynchronize(b->o.stream));
    if (const int cv = canary_verdict(b)) return cv;
    double ms[2] = {0, 0};
    pagan_batch_last_ms(b, ms);
    for (int k = 0; k < b->n; ++k) std::memset(&out[k], 0, sizeof(pagan_result));
    // copies first (one device queue), then the path replays of the jobs side by side on the host
    struct Fetched { int endcell[8]; double endscore; std::vector<int> trace; };
    std::vector<Fetched> got(b->n);
    std::vector<char> ends(kEndStride * (size_t)b->n);
    if (b->n > 0) HIP_TRY(hipMemcpy(ends.data(), b->arena.dev + b->end_off[0], ends.size(), hipMemcpyDeviceToHost));
    {
        // A visited cell whose stored back-pointer (or score) is not what its predecessors' scores give (pg_trace_check), or
        // a chase that ran into an impossible word: the batch runs once more with every back-pointer written by pg_backptr
        // after the fill -- the follower workgroups' early reads are the one thing a second run can take out.  What fails
        // again is reported.  PAGAN_DP_RERUN=0: report at once.
        bool again = false, score_again = false;
        for (int k = 0; k < b->n; ++k) {
            const int st = *reinterpret_cast<const int *>(ends.data() + kEndStride * (size_t)k);
            again = again || st == PG_STATUS_PATH_CHECK || st == 2;
            // a cell whose stored scores are not what its predecessors' stored scores give (PG_FLAG_SCORE_CHECK)
            if (st == (0x40000000 | PG_FILL_SCORE_MISMATCH)) { again = true; score_again = true; }
        }
        if (score_again)
            for (int k = 0; k < b->n; ++k) HIP_TRY(hipMemsetAsync(b->dj[k].fill_status, 0, sizeof(int), b->o.stream));
        // A strip that found the strip above on another XCD gave up (dp_pipe.hip, strip_feeder: tag 11): the strips' launch
        // once more with nothing dispatched beside it
        bool strips_again = false;
        for (int k = 0; k < b->n && !b->strips_alone; ++k) {
            const int st = *reinterpret_cast<const int *>(ends.data() + kEndStride * (size_t)k);
            if (b->jobs[k].route == STRIPS && (st & 0x40000000) && (st & PG_FILL_OTHER_XCD)) strips_again = true;
        }
        if (strips_again) {
            b->strips_alone = true;
            for (int k = 0; k < b->n; ++k)
                if (b->jobs[k].route == STRIPS) HIP_TRY(hipMemsetAsync(b->dj[k].fill_status, 0, sizeof(int), b->o.stream));
            again = true;
        }
        if (again && sw.rerun) {             // (once per fetch; the batch stays without followers)
            if (sw.verbose)
                std::fprintf(stderr, strips_again ? "pagan_dp: a row strip found the strip above on another XCD: running the batch again, the strips alone\n"
                                     : (score_again ? "pagan_dp: score check failed (a stored score is not what its predecessors give): running the batch again without follower workgroups\n"
                                                    : "pagan_dp: path check failed: running the batch again without follower workgroups\n"));
            if (!strips_again) b->no_follow = true;
            ++b->reruns;
            int rc = pagan_batch_run(b);
            if (rc != PAGAN_OK) return rc;
            HIP_TRY(hipStreamSynchronize(b->o.stream));
            pagan_batch_last_ms(b, ms);
            HIP_TRY(hipMemcpy(ends.data(), b->arena.dev + b->end_off[0], ends.size(), hipMemcpyDeviceToHost));
        }
    }
    for (int k = 0; k < b->n; ++k) {
        const int st = *reinterpret_cast<const int *>(ends.data() + kEndStride * (size_t)k);
        if (b->strips_alone && b->jobs[k].route == STRIPS && (st & 0x40000000) && (st & PG_FILL_OTHER_XCD)) b->strip_xcd_failure = true;
    }
    for (int k = 0; k < b->n; ++k) {
        Fetched &f = got[k];
        std::memcpy(f.endcell, ends.data() + kEndStride * (size_t)k, sizeof(f.endcell));
        std::memcpy(&f.endscore, ends.data() + kEndStride * (size_t)k + 32, sizeof(double));
        const int nt = f.endcell[0] == 0 ? f.endcell[6] : 0;
        if (nt < 0 || nt > b->jobs[k].Lx + b->jobs[k].Ly) return PAGAN_E_INTERNAL;
    }
    std::vector<int> rcs(b->n, PAGAN_OK);
    parallel_jobs(b->n, [&](int k) {
        // (a job's path comes over in its own thread: the copies' host sides -- page pinning, the staging copy -- overlap)
        {
            Fetched &f = got[k];
            const int nt = f.endcell[0] == 0 ? f.endcell[6] : 0;
            f.trace.resize(3 * (size_t)nt + 3);
            if (nt > 0) (void)hipSetDevice(b->device);              // (a new thread starts on device 0)
            if (nt > 0 && hipMemcpy(f.trace.data(), b->arena.dev + b->trace_off[k], sizeof(int) * 3 * (size_t)nt, hipMemcpyDeviceToHost) != hipSuccess) {
                (void)hipGetLastError();
                rcs[k] = PAGAN_E_NODEVICE;
                return;
            }
        }
        const CompactJob &cj = b->compact[k];
        if (cj.on && (got[k].endcell[0] == 0 || got[k].endcell[0] == 1)) {
            // the device's path in the caller's site numbers and edge-list positions, then the usual replay on the caller's graphs
            Fetched &f = got[k];
            const CompactSide &cl = cj.l, &cr = cj.r;
            const int ml = (int)cl.keep.size(), mr = (int)cr.keep.size();
            bool ok = true;
            auto site = [&](const CompactSide &c, int m_, int t) { if (t < 0 || t >= m_) { ok = false; return 0; } return c.keep[t]; };
            auto slot_of = [&](const CompactSide &c, int m_, int t, int k_) {
                if (t < 0 || t >= m_ || k_ < 0 || k_ >= c.off[t + 1] - c.off[t]) { ok = false; return 0; }
                return c.slot[c.off[t] + k_];
            };
            if (f.endcell[4] >= 0) f.endcell[4] = slot_of(cl, ml, ml - 1, f.endcell[4]);
            if (f.endcell[5] >= 0) f.endcell[5] = slot_of(cr, mr, mr - 1, f.endcell[5]);
            if (f.endcell[0] == 0) {
                f.endcell[2] = site(cl, ml, f.endcell[2]); f.endcell[3] = site(cr, mr, f.endcell[3]);
                const int nt = f.endcell[6];
                for (int t = 0; t < nt && ok; ++t) {
                    const int ci = f.trace[3 * t], cjx = f.trace[3 * t + 1];
                    const unsigned w_ = (unsigned)f.trace[3 * t + 2];
                    const int vit = (int)(w_ & 3u);
                    int k1 = (int)((w_ >> 4) & 16383u), k2 = (int)(w_ >> 18);
                    if (vit != PAGAN_Y_MAT) k1 = slot_of(cl, ml, ci, k1);
                    if (vit != PAGAN_X_MAT) k2 = slot_of(cr, mr, cjx, k2);
                    f.trace[3 * t] = site(cl, ml, ci); f.trace[3 * t + 1] = site(cr, mr, cjx);
                    f.trace[3 * t + 2] = (int)((w_ & 15u) | ((unsigned)k1 << 4) | ((unsigned)k2 << 18));
                }
            }
            if (!ok) { rcs[k] = PAGAN_E_INTERNAL; return; }
            HostJob orig;
            orig.L = cj.L0; orig.R = cj.R0; orig.Lx = cj.L0->n_sites - 1; orig.Ly = cj.R0->n_sites - 1;
            orig.dx.cells = cj.cells0;
            rcs[k] = replay(orig, f.endcell, f.endscore, f.trace.data(), sw.verbose, &out[k]);
            out[k].fill_ms = ms[0];
            out[k].trace_ms = ms[1];
            return;
        }
        rcs[k] = replay(b->jobs[k], got[k].endcell, got[k].endscore, got[k].trace.data(), sw.verbose, &out[k]);
        out[k].fill_ms = ms[0];
        out[k].trace_ms = ms[1];
    });
    int first_err = PAGAN_OK;
    for (int k = 0; k < b->n; ++k)
        if (rcs[k] != PAGAN_OK && first_err == PAGAN_OK) first_err = rcs[k];
    return first_err;
}

// Diagnostic: fill every output array of the batch (scores, back-pointers, traceback tables) with
// 0xFF bytes -- NaN scores -- so that a read of a cell that has not been written yet in THIS run
// cannot silently return the previous run's (identical) value.
int pagan_batch_debug_poison(pagan_batch *b) {
    if (!b) return PAGAN_E_ARG;
    HIP_TRY(hipMemsetAsync(b->arena.dev + b->out_begin, 0xFF, b->arena.size - b->out_begin, b->o.stream));
    return PAGAN_OK;
}

// Test hook: after the NEXT run's fill and before its traceback, state `vit` of cell (i, j) of job k gets `word` as its
// back-pointer (once).  tests/test_pipe_gpu.py corrupts a pointer on the path with it and expects the path check to see it.
int pagan_batch_debug_poke_bp(pagan_batch *b, int32_t k, int32_t i, int32_t j, int32_t vit, uint32_t word) {
    if (!b || k < 0 || k >= b->n) return PAGAN_E_ARG;
    b->poke[0] = k; b->poke[1] = i; b->poke[2] = j; b->poke[3] = vit; b->poke[4] = (int)word;
    return PAGAN_OK;
}
// How often pagan_batch_fetch ran the batch again after a failed path check.
int pagan_batch_debug_reruns(pagan_batch *b) { return b ? b->reruns : PAGAN_E_ARG; }

// Diagnostic: how many of job k's chunks of PG_FOLLOW_CHUNK diagonals had their back-pointers written behind the fill by
// the follower workgroups of pg_fill_pipe (the rest were left to pg_backptr); counts[0] = those, counts[1] = all chunks.
// A job of another kernel reports 0 of 0.
int pagan_batch_debug_followed(pagan_batch *b, int32_t k, int32_t *counts) {
    if (!b || k < 0 || k >= b->n || !counts) return PAGAN_E_ARG;
    counts[0] = counts[1] = 0;
    if (!b->dj[k].bp_done) return PAGAN_OK;
    HIP_TRY(hipStreamSynchronize(b->o.stream));
    const size_t n = ((size_t)b->dj[k].nd + PG_FOLLOW_CHUNK - 1) / PG_FOLLOW_CHUNK;
    std::vector<unsigned char> flags(n);
    HIP_TRY(hipMemcpy(flags.data(), b->dj[k].bp_done, n, hipMemcpyDeviceToHost));
    counts[1] = (int32_t)n;
    for (unsigned char f : flags) counts[0] += f != 0;
    return PAGAN_OK;
}

// Diagnostic: job k's score array, [cells][3] doubles in diagonal-major order (dp_device.h).
int pagan_batch_debug_scores(pagan_batch *b, int32_t k, double *dst, int64_t count) {
    if (!b || k < 0 || k >= b->n || !dst || count > 3 * b->jobs[k].dx.cells) return PAGAN_E_ARG;
    HIP_TRY(hipStreamSynchronize(b->o.stream));
    HIP_TRY(hipMemcpy(dst, b->dj[k].sc, sizeof(double) * (size_t)count, hipMemcpyDeviceToHost));
    return PAGAN_OK;
}

// Diagnostic: job k's back-pointer array, [cells][3] packed words (dp_device.h) in diagonal-major order.
int pagan_batch_debug_backptrs(pagan_batch *b, int32_t k, uint32_t *dst, int64_t count) {
    if (!b || k < 0 || k >= b->n || !dst || count > 3 * b->jobs[k].dx.cells) return PAGAN_E_ARG;
    HIP_TRY(hipStreamSynchronize(b->o.stream));
    HIP_TRY(hipMemcpy(dst, b->dj[k].bp, sizeof(uint32_t) * (size_t)count, hipMemcpyDeviceToHost));
    return PAGAN_OK;
}

// Diagnostic: raw copy of job k's trace buffer (used by tools/ with a -DPG_STAMPS build).
int pagan_batch_debug_trace(pagan_batch *b, int32_t k, void *dst, int64_t bytes) {
    if (!b || k < 0 || k >= b->n || !dst) return PAGAN_E_ARG;
    HIP_TRY(hipStreamSynchronize(b->o.stream));
    HIP_TRY(hipMemcpy(dst, b->arena.dev + b->trace_off[k], (size_t)bytes, hipMemcpyDeviceToHost));
    return PAGAN_OK;
}

// Diagnostic: how job k's last traceback was cut (pg_trace_compose's output; tests/trace_plan.py predicts it).  A download only.
int pagan_batch_debug_segments(pagan_batch *b, int32_t k, int32_t info[4], int32_t *segs, int64_t cap) {
    if (!b || k < 0 || k >= b->n || !info || cap < 0 || (cap > 0 && !segs) || !b->ran) return PAGAN_E_ARG;
    HIP_TRY(hipStreamSynchronize(b->o.stream));
    int ec[8];
    HIP_TRY(hipMemcpy(ec, b->dj[k].endcell, sizeof ec, hipMemcpyDeviceToHost));
    const int seg_cap = 2 * b->jobs[k].n_bound + 8;                    // (what pg_trace_compose stops at)
    int nseg = ec[0] == 0 ? ec[7] : 0;
    if (nseg < 0 || nseg > seg_cap) return PAGAN_E_INTERNAL;
    info[0] = b->jobs[k].n_bound; info[1] = nseg; info[2] = ec[0] == 0 ? ec[6] : 0; info[3] = ec[0];
    const int n = (int)std::min<int64_t>(nseg, cap);
    if (n > 0) {
        std::vector<int> raw(6 * (size_t)n);
        HIP_TRY(hipMemcpy(raw.data(), b->dj[k].segs, sizeof(int) * raw.size(), hipMemcpyDeviceToHost));
        for (int s = 0; s < n; ++s)
            for (int c = 0; c < 5; ++c) segs[5 * s + c] = raw[6 * (size_t)s + c];
    }
    return PAGAN_OK;
}

void pagan_batch_destroy(pagan_batch *b) {
    if (!b) return;
    if (b->o.stream) {
        (void)hipStreamSynchronize(b->o.stream);
        if (b->o.stream2) (void)hipStreamSynchronize(b->o.stream2);
        std::vector<std::pair<int, GpuObjs>> drop;
        if (b->o.ev_join) gpu_pool.give(b->device, b->o, 4, &drop);     // (the set is whole: ev_join is the last one made)
        else drop.emplace_back(b->device, b->o);
        destroy_objs(drop);
        b->o = GpuObjs();
    }
    give_slab(arena_pool, b->device, b->arena.dev, b->arena.cap);
    if (b->d_guards) { (void)hipFree(b->d_guards); (void)hipFree(b->d_canary); b->d_guards = nullptr; b->d_canary = nullptr; }
    // What is left is host memory only (plans, band indices, compaction maps: megabytes per alignment, milliseconds of
    // unmapping per level of a tree walk): freed by a background thread, off the caller's path.
    struct Reaper {
        std::mutex m;
        std::condition_variable cv;
        std::vector<pagan_batch *> q;
        bool stop = false;
        std::thread th;
        Reaper() : th([this] {
            for (;;) {
                std::vector<pagan_batch *> take;
                {
                    std::unique_lock<std::mutex> l(m);
                    cv.wait(l, [this] { return stop || !q.empty(); });
                    take.swap(q);
                    if (take.empty() && stop) return;
                }
                for (pagan_batch *x : take) delete x;
            }
        }) {}
        ~Reaper() { { std::lock_guard<std::mutex> l(m); stop = true; } cv.notify_one(); th.join(); }
        void give(pagan_batch *x) { { std::lock_guard<std::mutex> l(m); q.push_back(x); } cv.notify_one(); }
    };
    static Reaper reaper;
    reaper.give(b);
}

// pagan_dp_align_batch; allow_strips = false: its third attempt
static int align_batch(int32_t n, const pagan_job *jobs, const pagan_opts *opts, pagan_result *out, bool allow_strips) {
    if (!out || n < 0) return PAGAN_E_ARG;
    for (int k = 0; k < n; ++k) std::memset(&out[k], 0, sizeof(pagan_result));
    pagan_batch *b = nullptr;
    const DpSwitches sw = DpSwitches::read();
    const bool verbose = sw.verbose;
    auto now = [] { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    const double t0 = now();
    int rc = batch_create(n, jobs, opts, sw, allow_strips, &b);
    if (rc != PAGAN_OK) return rc;
    const double t1 = now();
    rc = pagan_batch_run(b);
    if (rc == PAGAN_OK) rc = pagan_batch_sync(b);
    const double t2 = now();
    if (rc == PAGAN_OK) rc = pagan_batch_fetch(b, out);
    const double t3 = now();
    if (rc != PAGAN_OK) for (int k = 0; k < n; ++k) pagan_result_free(&out[k]);   // a failed batch hands back nothing
    // Third attempt (round 4's advisor): row strips are only right when a job's strips run on one XCD, and the launch of the strips
    // "alone" is alone only within its batch -- another batch, thread or process on the device can still change where workgroups
    // land.  If that launch failed the same way, the batch is planned again with every wide job on the tiled kernel.
    const bool no_strips_now = rc == PAGAN_E_INTERNAL && b->strip_xcd_failure && allow_strips;
    pagan_batch_destroy(b);
    if (no_strips_now) {
        if (verbose) std::fprintf(stderr, "pagan_dp: the strips alone met another XCD again: the batch once more with its wide jobs on the tiled kernel\n");
        return align_batch(n, jobs, opts, out, false);
    }
    if (verbose)
        std::fprintf(stderr, "pagan_dp: batch of %d: create %.1f ms, kernels %.1f ms, fetch+replay %.1f ms, destroy %.1f ms\n", n,
                     1e3 * (t1 - t0), 1e3 * (t2 - t1), 1e3 * (t3 - t2), 1e3 * (now() - t3));
    return rc;
}

int pagan_dp_align_batch(int32_t n, const pagan_job *jobs, const pagan_opts *opts, pagan_result *out) {
    return align_batch(n, jobs, opts, out, true);
}

int pagan_dp_align(const pagan_graph *left, const pagan_graph *right, const pagan_model *model,
                   const pagan_band *band, const pagan_opts *opts, pagan_result *out) {
    pagan_job jb{left, right, model, band};
    return pagan_dp_align_batch(1, &jb, opts, out);
}

void pagan_dp_release_cache(void) {
    pagan::anchors_release_cache();
    pagan::parent_release_cache();
    pagan_fb_internal_release_cache();
    drain_slabs(arena_pool, -1);
    std::vector<std::pair<int, GpuObjs>> objs;
    gpu_pool.drain(&objs);
    destroy_objs(objs);
    std::lock_guard<std::mutex> g(stage_pool.m);
    for (auto &s : stage_pool.idle) std::free(s.first);
    stage_pool.idle.clear();
}

int64_t pagan_dp_cached_device_bytes(int32_t device) { return (int64_t)arena_pool.idle_bytes(device); }

void pagan_result_free(pagan_result *r) {
    if (!r) return;
    std::free(r->cols); std::free(r->left_used); std::free(r->right_used);
    r->cols = nullptr; r->left_used = nullptr; r->right_used = nullptr;
    r->n_cols = r->n_left_used = r->n_right_used = 0;
}

} // extern "C"
