// dp_fb_plan.h -- the forward/backward side's host-only planning (dp_fb_plan.cpp): the environment switches, the job record the
// kernels read, and the plan of one pair -- band index, corner initialisation, forward lists, the schedule its sweeps take with the
// deep-ring segments, the workgroup each schedule launches with, the decode route.  Plain C++17, no HIP: dp_fb.hip stages and
// launches what this plans, and everything here runs (and is tested, under sanitizers too: tests/native/fb_plan_main.cpp) without a
// device.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

#include "../../include/pagan_dp.h"
#include "dp_band.h"

// The constants plan and kernels share (dp_fb.hip and dp_fb_deep.inc say what the kernels do with them).
#define FB_T 64                 // side of a block of the block schedule
#define FB_MAX_GROUPS 64        // most workgroups of a tiled sweep
#define FB_RG_MAXB 1024         // rows of the widest diagonal a ring sweep takes
#define FB_RG_INIT 32           // assignments of initialise_array_corner_bwd a ring sweep holds (a pair with more takes the block schedule)
#define FB_RG_THREADS 1024      // B = 64 ... 256: three threads a row, one per state; B = 512: two (X and Y; M)
#define FB_DP_CELLS 4096        // D * B
#define FB_DP_W 1352            // sites in a window: <= 1,024 rows of a diagonal + FB_DP_REFILL + the 64 a near edge reaches ahead (backward)
#define FB_DP_E 1664            // list entries in a window (a pair with more in any FB_DP_W consecutive sites is not eligible)
#define FB_DP_MINSEG 256        // hysteresis of the segment plan, in diagonals
#define FB_DP_HALO 64           // diagonals either side that a diagonal's B must hold as well (>= any D - 1)

struct PgFbJob {
    int Lx, Ly, nd, S;
    double l_ext, l_open, l_ng;              // logs of gap_ext, gap_open, non_gap
    const int *stL, *offL, *srcL; const float *lwL;      // bwd lists (log weights as the CSR carries them)
    const int *stR, *offR, *srcR; const float *lwR;
    const int *foffL, *fdstL; const float *flwL;         // fwd lists
    const int *foffR, *fdstR; const float *flwR;
    const double *ltab;                      // log((double) score[a + b*S])
    const int *imin, *imax; const long long *doff;
    long long cells;
    double *F, *B;                           // [cells][3] log forward / log backward
    int n_init; const long long *init_at; const double *init_val;   // initialise_array_corner_bwd
    double *totals;                          // [2]: log fwd_end, log bwd(M,0,0)
    // the tiled sweeps (round 5: one launch may carry the sweeps of SEVERAL pairs, grid = (most workgroups of any pair, pairs) --
    // pagan_fb_run_batch): the pair's own workgroup count and barrier words
    int groups, groups_b;                    // workgroups of this pair's forward / backward sweep (blockIdx.x beyond: nothing to do)
    int *sync;                               // [64] ints: forward barrier at [0..7], backward at [8..15], diagnostics behind
    int init_dmin;                           // the first cell diagonal that holds a cell of init_at (nd: none)
    // the deep-ring sweeps (graph pairs inside a tunnel, dp_fb_deep.inc): the segments of the pair's diagonals
    int nseg; const int *seg_start;          // [nseg + 1] first diagonal of a segment, then nd
    const int *seg_B;                        // [nseg] rows B of the segment's workgroup layout | 1 << 16: the segment holds a far cell
    const int *dfar;                         // [nd] bit 0: the diagonal holds a cell with a far predecessor (forward), bit 1: a far successor (backward)
};

namespace fbplan {

// Every PAGAN_FB_* variable the library reads, parsed (INTEGRATION.md lists them by these names; tests/test_fb_plan_cpu.py holds the
// list against FbSwitches::read).  Read once per entry point -- pagan_fb_run_batch, pagan_fb_decode_batch, the host-only
// pagan_fb_debug_* calls -- and passed down; per call, not per process: tests flip variables between calls.
struct FbSwitches {
    // ---- the schedule of a pair's sweeps (fb_plan_pair) ----
    bool ring = true;                    // RING=0: long tunnels between plain sequences stay off the LDS-ring sweeps
    int ring_min_nd = 256;               // RING_MIN_ND: the shortest pair (in cell diagonals) that takes them
    bool ring_split = true;              // RING_SPLIT=0: a ring workgroup with one thread a row instead of one per state
    bool deep = true;                    // DEEP=0: graph pairs inside tunnels stay off the deep-ring sweeps
    int deep_min_nd = 4096;              // DEEP_MIN_ND: their shortest pair
    int band_min_nd = 4096;              // BAND_MIN_ND: the shortest narrow pair that takes the block schedule; =off: none
    bool groups_set = false;             // GROUPS (set at all): no ring, no deep ring, and ...
    int groups = 1;                      // GROUPS=n: ... n workgroups a tiled sweep, 1 ... FB_MAX_GROUPS (1: the one-workgroup kernels)
    // ---- the launches of a batch (fb_run_chunk) ----
    int slots_x16 = 46;                  // SLOTS_X16: sixteenths of a workgroup slot per compute unit in the tiled sweeps' budget, 8 ... 48
    int split = 40;                      // SPLIT: the forward sweeps' per cent of a pair's slots, 20 ... 80
    bool bwd_first = false;              // BWD_FIRST (set at all): the backward tiled sweep's workgroups are dealt out first
    // ---- the decode (pagan_fb_decode_batch) ----
    bool decode_ring = true;             // DECODE_RING=0: every decode matrix by pg_fb_decode_fill
    // ---- wherever it is read ----
    bool verbose = false;                // PAGAN_DP_VERBOSE (set at all)
    static FbSwitches read();
};

// the model's log scores sit in LDS (the kernels compiled without the table's load from memory)
inline bool fb_table_in_lds(int n_states) { return n_states * n_states <= 256; }

// A site's fwd list = its outgoing edges in creation order (Edge::index); the log weight is the bwd CSR's.
struct FwdLists { std::vector<int> off, dst; std::vector<float> lw; };
FwdLists forward_lists(const pagan_graph *g);

// Rows of the widest diagonal -> the 64 / 128 / 256 / 512 / 1,024 of a workgroup.  A ring, deep-ring or decode-ring workgroup has
// a row each: the smallest rung that holds `width`.  The one-workgroup kernels (`one_workgroup`: the sweeps, pg_fb_decode_fill)
// loop over a diagonal's cells and step up from 96, 192, 384 and 768 cells on: a thread with two cells of every diagonal was the
// sweep's pace.
int fb_block_for(int width, bool one_workgroup = false);

// Which kernel fills a pair's decode matrix: 1 = pg_fb_ring_decode -- two plain sequences whose widest diagonal fits a workgroup,
// the predicate of schedule 2 without its shortest-pair rule (there is no tiled alternative to win on a short pair) --, 0 =
// pg_fb_decode_fill.  Which sweep schedule wrote F and B does not matter: the layout is one.
int fb_decode_route(const pagan_graph *left, const pagan_graph *right, int Lx, int Ly, const DiagIndex &dx, const FbSwitches &sw);

// Everything that is decided about a pair before anything is allocated: fb_stage applies the caller's caps, lays out the arena
// and uploads; the host-only pagan_fb_debug_* calls return what is here.
struct FbPlan {
    int Lx = 0, Ly = 0, nd = 0;
    RowBand rb;                              // (the handle keeps these two: fb_stage moves them out)
    DiagIndex dx;
    // initialise_array_corner_bwd: index 3 * cell + state and value of every assignment onto the cells the end corner reads
    std::vector<long long> init_at;
    std::vector<double> init_val;
    int init_dmin = 0;                       // the first cell diagonal that holds a cell of init_at (nd: none)
    bool both_plain = false, gapless = false; // two plain sequences (every site one edge, from the site before it); no cell diagonal without a cell
    FwdLists fl, fr;
    // the schedule (codes of pagan_fb_schedule): 0 one workgroup, 1 tiled, 2 ring, 3 deep ring
    int groups = 1;                          // workgroups of a tiled sweep before the caller's caps (1: not tiled)
    bool ring = false, deep = false;
    int info[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // see pagan_fb_debug_route
    std::vector<int> seg_start, seg_B, dfar; // the deep-ring plan (PgFbJob has the layout); empty unless deep
    int schedule() const { return deep ? 3 : (ring ? 2 : (groups > 1 ? 1 : 0)); }
    // what the sweeps launch with: the threads of a one-workgroup, tiled or deep-ring workgroup, the rows B of a ring sweep's, whose
    // workgroup has `nsplit` threads a row
    int block = 64, nsplit = 1;
    // a tiled sweep's workgroups within what the caller's launch leaves it
    int groups_within(int cap) const { return groups > 1 ? std::max(2, std::min(groups, cap)) : 1; }
    int decode_route = 0, decode_block = 64; // fb_decode_route, and the rows (1) or threads (0) of its workgroup
};

// Checks both graphs and the band and plans the pair under `sw`; l_ng: the model's log non_gap, which only the values of the
// corner's assignments depend on.  PAGAN_OK or a negative PAGAN_E_*.
int fb_plan_pair(const pagan_graph *left, const pagan_graph *right, const pagan_band *band, const FbSwitches &sw, FbPlan *plan, double l_ng = 0.0);

} // namespace fbplan
