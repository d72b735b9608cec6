// dp_abi.hip -- the C ABI of include/pagan_dp.h on top of the gfx950 kernels.
//
// Host work done here is bookkeeping only: validate the borrowed inputs, turn the row band
// (upper/lower per left site, the reference's "tunnel") into the per-anti-diagonal index the
// kernels use, stage everything into ONE device arena per batch, launch, and turn the
// device's list of visited path cells into the reference's path (skip columns + used edges,
// Viterbi_alignment::backtrack_new_path, src/main/viterbi_alignment.cpp:1038-1189).
// There is no CPU fill or traceback here: without a HIP device every entry point fails.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <thread>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <condition_variable>
#include <mutex>
#include <new>
#include <type_traits>
#include <vector>
#include <unordered_map>

#include "host_anchors.h"
#include "host_graph.h"
#include "../../include/pagan_dp.h"
#include "dp_device.h"
#include "dp_band.h"

template <int BLOCK> __global__ void pg_fill_wavefront(const PgDevJob *jobs, const int *which, unsigned flags);
template <bool TAB_LDS> __global__ void pg_fill_ring(const PgDevJob *jobs, const int *which, unsigned flags);
template <bool TAB_LDS, bool STRIP> __global__ void pg_fill_pipe(const PgDevJob *jobs, const int *which, unsigned flags, int n_fill);
__global__ void pg_fill_tiles(const PgDevJob *jobs, const int *tiles, unsigned flags);
__global__ void pg_fill_tiles_flow(const PgDevJob *jobs, const int *tiles, int n_tiles, int n_diag, int *flow, unsigned flags, int use_water);
__global__ void pg_end_corner(const PgDevJob *jobs, const int *tiles_gave_up);
__global__ void pg_backptr(const PgDevJob *jobs, const int *which, unsigned flags, int diags_per_block);
__global__ void pg_trace_spec(const PgDevJob *jobs);
__global__ void pg_trace_compose(const PgDevJob *jobs);
__global__ void pg_trace_emit(const PgDevJob *jobs);
__global__ void pg_trace_check(const PgDevJob *jobs, unsigned flags);
__global__ void pg_debug_poke_bp(const PgDevJob *jobs, int k, int i, int j, int vit, unsigned word);

// limits of the LDS-staged kernel (dp_kernels.hip: RW site window, EC edge ring)
#define PG_RING_MAX_WIDTH 256
#define PG_RING_SITE_SPAN 576
// a diagonal fewer than this behind a wide one is a general step (classify_diagonals); PAGAN_DP_AFTER_WIDE=reach: REACH, as before round 5 (A/B switch)
static int pg_after_wide() {      // (read per plan, not once per process: the tests switch it)
    const char *e = std::getenv("PAGAN_DP_AFTER_WIDE");
    return (e && std::strcmp(e, "reach") == 0) ? PG_PIPE_REACH : 3;
}
#define PG_RING_EDGE_CAP 2048
unsigned pg_ring_lds_bytes();
// limits of the register-wavefront kernel: PG_PIPE_* in dp_device.h, shared with dp_pipe.hip
unsigned pg_pipe_lds_bytes();        // (static LDS: reported, not passed at launch)
unsigned pg_pipe_block();
unsigned pg_tiles_lds_bytes();

extern "C" void pagan_fb_internal_release_cache();             // dp_fb.hip: the forward/backward arenas kept for the next pair

namespace {

#define HIP_TRY(expr)                                                                            \
    do {                                                                                         \
        hipError_t e__ = (expr);                                                                 \
        if (e__ != hipSuccess) {                                                                 \
            if (std::getenv("PAGAN_DP_VERBOSE"))                                                 \
                std::fprintf(stderr, "pagan_dp: %s failed: %s\n", #expr, hipGetErrorString(e__)); \
            return e__ == hipErrorOutOfMemory ? PAGAN_E_NOMEM : PAGAN_E_NODEVICE;                \
        }                                                                                        \
    } while (0)

inline size_t align_up(size_t x, size_t a = 256) { return (x + a - 1) / a * a; }

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
    // far histories (dp_pipe.hip, PipeSmem::hist; plan_far_hist below): per site of either graph a flag byte, per diagonal
    // whether a reader or a writer of a history line has a cell on it; all empty when the job has none
    std::vector<uint8_t> hfL, hfR, hbit;
    std::vector<uint8_t> tbit;   // per diagonal: a three-edge site the lanes take in a third pass has a cell on it (empty: none)
    std::vector<int> tiles;      // dp_tiles.hip (jobs that are not ring_ok): tile row, tile column of every tile that may hold a cell
    std::vector<struct StripPlan> strips;   // dp_pipe.hip, row strips (jobs that are not ring_ok and qualify: plan_strips); empty otherwise
    int n_bound = 0;             // traceback boundaries (dp_device.h)
    std::vector<int> tb;         // [n_bound + 2] table offsets
};

// The ring kernel keeps the bwd edges of ~256 consecutive sites in a 1024-entry LDS ring.
bool edges_fit_ring(const pagan_graph *g, int rows, int cap = PG_RING_EDGE_CAP, int per_site = PG_MAX_SLOT) {
    for (int i = 0; i < rows; ++i) {
        const int e = i + PG_RING_SITE_SPAN < rows ? i + PG_RING_SITE_SPAN : rows;
        if (g->bwd_off[e] - g->bwd_off[i] > cap) return false;
        if (g->bwd_off[i + 1] - g->bwd_off[i] > per_site) return false;
    }
    return true;
}

bool has_negative_zero(const pagan_job &jb) {
    auto neg0 = [](float f) { return f == 0.0f && std::signbit(f); };
    const pagan_model *m = jb.model;
    if (neg0(m->log_gap_open) || neg0(m->log_gap_ext) || neg0(m->log_gap_end_ext) || neg0(m->log_non_gap)) return true;
    for (int k = 0; k < m->n_states * m->n_states; ++k) if (neg0(m->log_score[k])) return true;
    for (const pagan_graph *g : {jb.left, jb.right})
        for (int k = 0; k < g->bwd_off[g->n_sites]; ++k) if (neg0(g->bwd_logw[k])) return true;
    return false;
}

// What the fill kernel may assume about a site without looking at its edge list.
struct SiteFeat {
    std::vector<int> span;            // farthest bwd edge, in sites (0: no bwd edge)
    std::vector<int> span_ring;       // farthest bwd edge that reaches fewer than PG_PIPE_REACH sites back (>= 1)
    std::vector<int> not_simple;      // prefix count of sites that are not "one edge from the previous site, weight 1"
    std::vector<int> no_pred;         // prefix count of sites without bwd edges
    std::vector<int> not_easy;        // prefix count of sites the compute waves of dp_pipe.hip do not evaluate themselves: anything
                                      // but one edge from the previous site (any weight), alone or beside ONE edge from further back
    // (round 5) a site with THREE edges, one of them from the previous site and the other two inside the ring's reach (the pair
    // operand of an edge k sites back is k + 1 diagonals old): the lanes evaluate it in a third pass of their class 1 blocks
    // (tools/gen_hot_asm.py, third_pass).  not_easy3 / three: prefix counts -- not_easy without those sites, and those sites.
    std::vector<int> not_easy3, three;
    std::vector<uint8_t> is_three;
    // first_simple (row strips): site 0 passes for a simple site (dp_pipe.hip, load_rec_chunk)
    void build(const pagan_graph *g, int n, bool first_simple = false) {
        span.assign(n, 0); span_ring.assign(n, 1); not_simple.assign(n + 1, 0); no_pred.assign(n + 1, 0); not_easy.assign(n + 1, 0);
        not_easy3.assign(n + 1, 0); three.assign(n + 1, 0); is_three.assign(n, 0);
        for (int s = 0; s < n; ++s) {
            if (s == 0 && first_simple) continue;
            const int a = g->bwd_off[s], b = g->bwd_off[s + 1];
            int sp = 0, spr = 1;
            for (int k = a; k < b; ++k) {
                const int dist = s - g->bwd_src[k];
                sp = std::max(sp, dist);
                if (dist < PG_PIPE_REACH) spr = std::max(spr, dist);
            }
            span[s] = sp; span_ring[s] = spr;
            const bool simple = s > 0 && b - a == 1 && g->bwd_src[a] == s - 1 && g->bwd_logw[a] == 0.0f;
            not_simple[s + 1] = not_simple[s] + (simple ? 0 : 1);
            no_pred[s + 1] = no_pred[s] + (b == a ? 1 : 0);
            int n_adj = 0;
            for (int k = a; k < b; ++k) n_adj += g->bwd_src[k] == s - 1;
            const bool easy = s > 0 && (b - a == 1 || b - a == 2) && n_adj == 1;
            not_easy[s + 1] = not_easy[s] + (easy ? 0 : 1);
            const bool th = s > 0 && b - a == 3 && n_adj == 1 && sp <= PG_PIPE_REACH - 2;
            is_three[s] = th;
            three[s + 1] = three[s] + (th ? 1 : 0);
            not_easy3[s + 1] = not_easy3[s] + ((easy || th) ? 0 : 1);
        }
    }
};

// Class of every anti-diagonal for dp_pipe.hip (its header explains the five code paths):
//   5  wider than PG_PIPE_WINDOW cells;   4  wider than PG_PIPE_WIDTH cells;
//   3  touches the first/last two rows or columns, holds a site without bwd edges, or follows a wide
//      diagonal within the ring's reach;
//   2  holds a cell (i,j) whose farthest predecessor pair lies span(i) + span(j) >= PG_PIPE_REACH
//      diagonals back, or a multi-edge site within PG_PIPE_REACH rows/columns of the matrix's first (an edge
//      in reach may start at site 0, where the gap-open term differs);
//   1  holds a site that is not simple;   0  otherwise.
// `inwave` (model table in LDS): the compute waves evaluate the multi-edge cells of a class 1 diagonal themselves, which
// covers sites with one edge from the previous site and at most one more ("easy", SiteFeat::not_easy); a diagonal that
// holds any other multi-edge site is class 2 (the assist waves stage its candidates, ring-resident operands included).
// ---- far histories (round 5) -------------------------------------------------------------------------------------
// A site with one edge from the previous site and ONE other edge that reaches k >= PG_PIPE_REACH - 1 sites back reads cells
// that have left the LDS ring: until round 5 every diagonal such a site has a cell on was class 2 -- staged by an assist wave
// from L2, 2,600 cycles a step against a class 1 step's 1,100 (cfg4's root: 30 k of its 54 k class 2 diagonals are there for
// nothing else).  The cells such an edge reads are cells of ONE earlier row (column) -- the edge's start site p = s - k --
// taken k diagonals after they were computed.  So the lane that computes row p (a column's cell passes from lane to lane)
// also appends its cell, every step, to a HISTORY LINE in LDS -- 64 entries, indexed by the cell's column (row) modulo 64 --
// and the site's lane reads its operands there: an LDS read in place of a trip to L2, in the lanes that own the cell.
//
// This planner names the (start site -> far site) pairs that get a line: PG_HIST_SLOTS lines exist, a pair holds one from
// the first diagonal its start site has a cell on to the last diagonal of the far site (interval colouring in order of the
// first diagonal; a start site that several far sites share keeps one line).  A pair is served only if
//   * the far site is "easy" (one edge from the previous site + this one) and k <= PG_HIST_MAX_SPAN: an entry lives 64
//     steps, the reader comes k (+1) steps after the writer, and the waves of a workgroup are up to a ring's depth apart;
//   * the start site is not site 0 (an edge from site 0 opens a gap for free: the general rules);
//   * every diagonal of the interval runs in the hand-scheduled loop (class <= 2): the general steps and the wide runs write
//     no history.
// Flags per site (hfL / hfR, uploaded beside the graph; the loader stages them with the site records and sets PR_FAR in
// the far site's record): bit 7 reader + bits 0-1 its line, bit 6 writer + bits 4-5 its line.  hbit[d] = 1 on every
// diagonal of a served interval: the loop looks at the flags only there.  A cell where a far site meets a site that has an
// other edge of its own would need the pair of the two other edges as well: those single diagonals stay class 2 (marked by
// the caller through `cross`).  What is not served is marked far as before (class 2).
struct FarPlan {
    std::vector<uint8_t> tbit;                 // per diagonal: a three-edge site the lanes take in a third pass has a cell on it (classify_diagonals)
    std::vector<uint8_t> hfL, hfR, hbit;
    std::vector<uint8_t> servedL, servedR;     // per site: its far edge reads a history line
    int n_served = 0, n_hard = 0;
};

void plan_far_hist(const pagan_graph *L, const pagan_graph *R, int Lx, int Ly, const RowBand &rb, const DiagIndex &dx,
                   const SiteFeat &fl, const SiteFeat &fr, FarPlan *out) {
    const int nd = Lx + Ly - 1;
    out->hfL.assign(Lx, 0); out->hfR.assign(Ly, 0); out->hbit.assign(nd, 0);
    out->servedL.assign(Lx, 0); out->servedR.assign(Ly, 0);
    out->n_served = out->n_hard = 0;
    if (const char *e = std::getenv("PAGAN_DP_HIST")) if (std::strcmp(e, "0") == 0) return;      // A/B switch: every far site as before
    // diagonals that do not run in the hand-scheduled loop whatever the sites are (classify_diagonals has the rules)
    std::vector<int> slow(nd + 1, 0);
    {
        const int after_wide = pg_after_wide();
        // (round 5) the wide runs and the general steps behind them append to the history lines like the loop does (wide_run7,
        // wide_run, the kernel's general step): an interval may cross them; only class 5 diagonals -- and the steps behind THOSE --
        // write no history.  PAGAN_DP_HIST=narrow: as before (A/B).
        const char *he = std::getenv("PAGAN_DP_HIST");
        const bool hist_wide = !(he && std::strcmp(he, "narrow") == 0);
        int last_wide = -1000, last_wide5 = -1000;
        for (int d = 0; d < nd; ++d) {
            const int lo = dx.imin[d], hi = dx.imax[d];
            bool c3 = false;
            if (hi - lo + 1 > PG_PIPE_WIDTH) { c3 = hist_wide ? hi - lo + 1 > PG_PIPE_WINDOW : true; last_wide = d; if (hi - lo + 1 > PG_PIPE_WINDOW) last_wide5 = d; }
            else if (d - last_wide < after_wide) c3 = !hist_wide || d - last_wide5 < after_wide;
            else if (!(lo >= 2 && hi <= Lx - 2 && d - hi >= 2 && d - lo <= Ly - 2)) c3 = true;
            slow[d + 1] = slow[d] + (c3 ? 1 : 0);
        }
    }
    struct Cand { int start, end, site, src; bool left; };
    std::vector<Cand> cands;
    auto other_edge = [](const pagan_graph *g, int s, int *k) {      // easy two-edge site: the distance of the edge that is not from s - 1
        const int a = g->bwd_off[s], b = g->bwd_off[s + 1];
        if (s < 1 || b - a != 2) return false;
        const int d0 = s - g->bwd_src[a], d1 = s - g->bwd_src[a + 1];
        if ((d0 == 1) == (d1 == 1)) return false;
        *k = d0 == 1 ? d1 : d0;
        return true;
    };
    for (int i = 1; i < Lx; ++i) {
        int k;
        if (fl.span[i] < PG_PIPE_REACH - 1 || rb.hi[i] < rb.lo[i]) continue;
        if (!other_edge(L, i, &k) || k > PG_HIST_MAX_SPAN || i - k < 1 || rb.hi[i - k] < rb.lo[i - k]) { ++out->n_hard; continue; }
        cands.push_back({(i - k) + rb.lo[i - k] - 1, i + rb.hi[i] + 1, i, i - k, true});
    }
    for (int j = 1; j < Ly; ++j) {
        int k;
        if (fr.span[j] < PG_PIPE_REACH - 1) continue;
        // rows whose band holds a column: hi[] and lo[] are monotone
        auto rows_of = [&](int c, int *i1, int *i2) {
            *i1 = (int)(std::lower_bound(rb.hi.begin(), rb.hi.end(), c) - rb.hi.begin());
            *i2 = (int)(std::upper_bound(rb.lo.begin(), rb.lo.end(), c) - rb.lo.begin()) - 1;
        };
        int a1, a2, b1, b2;
        rows_of(j, &a1, &a2);
        if (a2 < a1) continue;                                     // (the column has no cell in the band)
        if (!other_edge(R, j, &k) || k > PG_HIST_MAX_SPAN || j - k < 1) { ++out->n_hard; continue; }
        rows_of(j - k, &b1, &b2);
        if (b2 < b1) { ++out->n_hard; continue; }
        cands.push_back({b1 + (j - k) - 1, a2 + j + 1, j, j - k, false});
    }
    std::stable_sort(cands.begin(), cands.end(), [](const Cand &x, const Cand &y) { return x.start < y.start; });
    struct Line { int end = -1000000; int src = -1; bool left = false; };
    Line lines[PG_HIST_SLOTS];
    for (const Cand &c : cands) {
        const int s0 = std::max(c.start, 0), s1 = std::min(c.end, nd - 1);
        int slot = -1;
        if (slow[s1 + 1] - slow[s0] == 0) {
            for (int q = 0; q < PG_HIST_SLOTS && slot < 0; ++q)       // the start site's line, if it has one that is still alive
                if (lines[q].src == c.src && lines[q].left == c.left && lines[q].end >= c.start) slot = q;
            for (int q = 0; q < PG_HIST_SLOTS && slot < 0; ++q) if (lines[q].end < c.start) slot = q;          // (a free line; what its last user left is never read: an operand in the band is always the present writer's)
        }
        if (slot < 0) { ++out->n_hard; continue; }
        lines[slot].end = std::max(lines[slot].end, c.end); lines[slot].src = c.src; lines[slot].left = c.left;
        std::vector<uint8_t> &hf = c.left ? out->hfL : out->hfR;
        hf[c.site] = (uint8_t)((hf[c.site] & 0x7c) | 0x80 | slot);
        hf[c.src] = (uint8_t)((hf[c.src] & 0x8f) | 0x40 | (slot << 4));
        (c.left ? out->servedL : out->servedR)[c.site] = 1;
        for (int d = s0; d <= s1; ++d) out->hbit[d] = 1;
        ++out->n_served;
    }
}

// f(first, last) over [0, n) cut into `threads` ranges, one thread each (the caller's thread takes the first)
template <class F> void par_ranges(int n, int threads, F f) {
    threads = std::max(1, std::min(threads, n / 4096));          // (a range below a few thousand items is not worth a thread)
    if (threads <= 1) { f(0, n); return; }
    std::vector<std::thread> pool;
    const int step = (n + threads - 1) / threads;
    for (int t = 1; t < threads; ++t) pool.emplace_back([&, t] { f(std::min(n, t * step), std::min(n, (t + 1) * step)); });
    f(0, std::min(n, step));
    for (auto &th : pool) th.join();
}

// `threads`: the plan of ONE alignment over several host threads (round 5: at the top of a guide tree a level holds one or two
// alignments, and their plans -- 7 ms each for 2 x 100 kb -- were serial host time between two kernels).  The site features of
// the two graphs are built side by side; the passes over the diagonals (class, ring residency, reach, ring-row reuse) run over
// ranges of diagonals: what couples the diagonals -- the running count of far cells, the last wide diagonal -- is two prefix
// passes done first; the sliding windows restart at a range's first diagonal by binary search.
void classify_diagonals(const pagan_graph *L, const pagan_graph *R, int Lx, int Ly, const RowBand &rb,
                        const DiagIndex &dx, bool inwave, std::vector<uint8_t> *out, std::vector<int> *lead_req,
                        std::vector<uint8_t> *ring2 = nullptr, int threads = 1, FarPlan *far_plan = nullptr) {
    const int nd = Lx + Ly - 1;
    static const bool prof = std::getenv("PAGAN_DP_PLAN_PROFILE") != nullptr;
    auto t_last = std::chrono::steady_clock::now();
    auto lap = [&](const char *what) {
        if (!prof) return;
        const auto t = std::chrono::steady_clock::now();
        std::fprintf(stderr, "pagan_dp:   classify: %s %.2f ms\n", what, std::chrono::duration<double, std::milli>(t - t_last).count());
        t_last = t;
    };
    SiteFeat fl, fr;
    if (threads > 1) {
        std::thread other([&] { fr.build(R, Ly); });
        fl.build(L, Lx);
        other.join();
    } else { fl.build(L, Lx); fr.build(R, Ly); }
    lap("site features");
    // far histories (plan_far_hist): which far sites read their operands from a history line instead of making their
    // diagonals class 2 (hand-scheduled loop only: `inwave`)
    FarPlan none;
    FarPlan &fp = far_plan ? *far_plan : none;
    if (far_plan && inwave) plan_far_hist(L, R, Lx, Ly, rb, dx, fl, fr, far_plan);
    else { fp.servedL.assign(Lx, 0); fp.servedR.assign(Ly, 0); fp.hbit.assign(nd, 0); }
    lap("far histories");
    // three-edge sites in the lanes (hand-scheduled loop, with a plan that can carry the per-diagonal bit)
    const bool three_ok = far_plan && inwave && !(std::getenv("PAGAN_DP_THREE") && std::strcmp(std::getenv("PAGAN_DP_THREE"), "0") == 0);
    const std::vector<int> &ne_l = three_ok ? fl.not_easy3 : fl.not_easy, &ne_r = three_ok ? fr.not_easy3 : fr.not_easy;
    if (far_plan) far_plan->tbit.assign(nd, 0);
    std::vector<int> far(nd + 1, 0), far2;
    std::vector<int> multi_cols, three_cols;           // columns with span >= 2 / three-edge columns, ascending
    for (int j = 0; j < Ly; ++j) if (fr.span[j] >= 2) multi_cols.push_back(j);
    if (three_ok) for (int j = 0; j < Ly; ++j) if (fr.is_three[j]) three_cols.push_back(j);
    // far_any: a far site (served by a history line or not) has a cell on the diagonal -- a class 2 diagonal then is not one
    // "whose operands all lie in the ring" even if the lanes' own far blocks would have taken the site on a class 1 diagonal
    std::vector<int> far_any_r(nd + 1, 0), far_any_c(nd + 1, 0);
    auto mark_rows = [&](std::vector<int> &fa) {
        auto mark = [&](int d0, int d1) { if (d0 <= d1) { ++fa[d0]; --fa[d1 + 1]; } };
        auto mark_any = [&](int d0, int d1) { if (d0 <= d1) { ++far_any_r[d0]; --far_any_r[d1 + 1]; } };
        for (int i = 0; i < Lx; ++i) {
            if (rb.hi[i] < rb.lo[i]) continue;
            const int sl = fl.span[i];
            if (three_ok && fl.is_three[i])         // a cell where two three-edge sites meet: the pairs of their second other edges are nobody's in the lanes
                for (auto it = std::lower_bound(three_cols.begin(), three_cols.end(), rb.lo[i]); it != three_cols.end() && *it <= rb.hi[i]; ++it) mark(i + *it, i + *it);
            if (sl >= PG_PIPE_REACH - 1) {
                mark_any(i + rb.lo[i], i + rb.hi[i]);
                if (!fp.servedL[i]) { mark(i + rb.lo[i], i + rb.hi[i]); continue; }   // any column: span(j) >= 1
                // its other edge reads a history line: only the cells where it meets a column with an other edge of its own
                // (the pair of the two other edges is not in the line's reach) stay with the assist waves
                for (auto it = std::lower_bound(multi_cols.begin(), multi_cols.end(), rb.lo[i]);
                     it != multi_cols.end() && *it <= rb.hi[i]; ++it) mark(i + *it, i + *it);
                continue;
            }
            if (sl < 2) continue;                          // with span(i) <= 1 only span(j) >= REACH-1 matters: below
            for (auto it = std::lower_bound(multi_cols.begin(), multi_cols.end(), rb.lo[i]);
                 it != multi_cols.end() && *it <= rb.hi[i]; ++it)
                if (sl + fr.span[*it] >= PG_PIPE_REACH) mark(i + *it, i + *it);
        }
    };
    auto mark_cols = [&](std::vector<int> &fa) {
        auto mark = [&](int d0, int d1) { if (d0 <= d1) { ++fa[d0]; --fa[d1 + 1]; } };
        auto mark_any = [&](int d0, int d1) { if (d0 <= d1) { ++far_any_c[d0]; --far_any_c[d1 + 1]; } };
        for (int j = 0; j < Ly; ++j) {
            if (fr.span[j] < PG_PIPE_REACH - 1) continue;
            // rows whose band holds column j: hi[] and lo[] are monotone
            const int i1 = (int)(std::lower_bound(rb.hi.begin(), rb.hi.end(), j) - rb.hi.begin());
            const int i2 = (int)(std::upper_bound(rb.lo.begin(), rb.lo.end(), j) - rb.lo.begin()) - 1;
            mark_any(i1 + j, i2 + j);
            if (!fp.servedR[j]) { mark(i1 + j, i2 + j); continue; }
            for (int i = std::max(i1, 0); i <= i2 && i < Lx; ++i) if (fl.span[i] >= 2) mark(i + j, i + j);     // (as for the rows: where it meets another other edge)
        }
    };
    if (threads > 1) {
        far2.assign(nd + 1, 0);
        std::thread other([&] { mark_cols(far2); });
        mark_rows(far);
        other.join();
        for (int d = 0; d <= nd; ++d) far[d] += far2[d];
    } else { mark_rows(far); mark_cols(far); }
    lap("far marks");
    out->assign(nd, 0);
    if (ring2) ring2->assign(nd, 0);
    // what couples the diagonals: far cells in flight (a running sum) and the last wide diagonal at or before d
    std::vector<int> run_at(nd), last_wide_at(nd), any_at(nd);
    {
        int run = 0, last_wide = -1000, any = 0;
        for (int d = 0; d < nd; ++d) {
            run += far[d];
            any += far_any_r[d] + far_any_c[d];
            if (dx.imax[d] - dx.imin[d] + 1 > PG_PIPE_WIDTH) last_wide = d;
            run_at[d] = run; last_wide_at[d] = last_wide; any_at[d] = any;
        }
    }
    // How far back in the LDS ring the cells of a diagonal read: 2 for simple cells, span(i) + span(j) for a
    // multi-edge cell (bounded here by the largest spans among the diagonal's rows and columns: sliding-window
    // maxima, both windows only move forward), the full reach for the other classes.  From that, the diagonal
    // the downstream wave must have completed before a wave may overwrite ring row D % PG_PIPE_RING with
    // diagonal D: the last diagonal that still reads D - PG_PIPE_RING.
    //
    // What matters for the reuse of a ring row is how far back the cells of a diagonal read IN ANOTHER
    // WAVE'S ROWS (a wave's reads of its own rows are ordered with its own writes).  A cell (i,j) reads rows
    // down to i - dL, so it crosses into the block of 64 rows above only if span_ring(i) > i % 64 -- lane 0
    // always does (row i-1: its shift operand at age 1 and the M operands at ages 1 + dR).  Such a cell
    // reaches at most span_ring(i) + span_ring(j) diagonals back in the ring (classes 1 and 2; older operands
    // come from L2).  Candidates per diagonal: the rows with a ring-reaching skip edge (sliding window over
    // their sorted list) and the at most four rows with i % 64 == 0.
    lap("prefix passes");
    std::vector<int> rowsL;
    for (int i = 0; i < Lx; ++i) if (fl.span_ring[i] >= 2) rowsL.push_back(i);
    std::vector<int> need(nd, PG_PIPE_REACH - 1);
    const int after_wide = pg_after_wide();
    par_ranges(nd, threads, [&](int d_first, int d_last) {
        for (int d = d_first; d < d_last; ++d) {
            const int run = run_at[d];
            const int lo = dx.imin[d], hi = dx.imax[d];
            uint8_t c;
            // Behind a wide diagonal (the ring's memory was the wide ring): pg_after_wide() - 1 = two general steps -- the first leaves the
            // lane's cell in registers and in the ring, the second also the shifted cell of the one before, which is what the
            // hand-scheduled loop starts from --, then the loop again (round 5; it used to be REACH - 1 general steps, ~5.6 us each):
            // a diagonal less than REACH behind the wide one that holds a multi-edge cell is class 2, and its residency mask
            // (descriptor word 4) sends the operands older than the general steps to L2 through the assist waves.
            const bool near_wide = d - last_wide_at[d] < PG_PIPE_REACH;
            if (hi - lo + 1 > PG_PIPE_WIDTH) c = hi - lo + 1 > PG_PIPE_WINDOW ? 5 : 4;
            else if (d - last_wide_at[d] < after_wide) c = 3;
            else if (!(lo >= 2 && hi <= Lx - 2 && d - hi >= 2 && d - lo <= Ly - 2)) c = 3;
            else if (run > 0) c = 2;
            else if ((lo < PG_PIPE_REACH || d - hi < PG_PIPE_REACH || near_wide) &&
                     (fl.not_simple[hi + 1] - fl.not_simple[lo] > 0 || fr.not_simple[d - lo + 1] - fr.not_simple[d - hi] > 0)) c = 2;
            else if (fl.not_simple[hi + 1] - fl.not_simple[lo] > 0 || fr.not_simple[d - lo + 1] - fr.not_simple[d - hi] > 0)
                c = (inwave && (ne_l[hi + 1] - ne_l[lo] > 0 || ne_r[d - lo + 1] - ne_r[d - hi] > 0)) ? 2 : 1;
            else c = 0;
            if (three_ok && c == 1 && (fl.three[hi + 1] - fl.three[lo] > 0 || fr.three[d - lo + 1] - fr.three[d - hi] > 0)) far_plan->tbit[d] = 1;
            if (c == 0 && fp.hbit[d]) c = 1;       // a history line's writer (or reader) has a cell here: the step looks at the sites' flags
            // a class 2 diagonal whose operands all lie in the ring (it is class 2 for the shape of a site only): the assist waves
            // take their ring-only code for it
            if (ring2) (*ring2)[d] = c == 2 && run == 0 && any_at[d] == 0 && !(lo < PG_PIPE_REACH || d - hi < PG_PIPE_REACH) && !near_wide;
            (*out)[d] = c;
        }
        // (the windows over the rows with a ring-reaching skip edge only move forward: they restart at the range's first diagonal)
        size_t la = 0, lb = 0;
        bool started = false;
        for (int d = d_first; d < d_last; ++d) {
            const int lo = dx.imin[d], hi = dx.imax[d];
            if (hi < lo || (*out)[d] > 2) continue;
            if (!started) {
                la = (size_t)(std::lower_bound(rowsL.begin(), rowsL.end(), lo) - rowsL.begin());
                lb = la;
                started = true;
            }
            while (lb < rowsL.size() && rowsL[lb] <= hi) ++lb;
            while (la < lb && rowsL[la] < lo) ++la;
            int m = 2;
            for (size_t k = la; k < lb; ++k) {
                const int i = rowsL[k];
                if (fl.span_ring[i] > (i & 63)) m = std::max(m, fl.span_ring[i] + fr.span_ring[d - i]);
            }
            for (int i = (lo + 63) & ~63; i <= hi; i += 64) m = std::max(m, fl.span_ring[i] + fr.span_ring[d - i]);
            need[d] = std::min(m, PG_PIPE_REACH - 1);
        }
    });
    lap("classes and reach");
    lead_req->assign(nd, -1);
    par_ranges(nd, threads, [&](int d_first, int d_last) {
        for (int D = std::max(d_first, (int)PG_PIPE_RING); D < d_last; ++D) {
            int req = -1;
            for (int t = D - PG_PIPE_RING + 1; t <= D - PG_PIPE_RING + PG_PIPE_REACH - 1 && t < nd; ++t)
                if (t - need[t] <= D - PG_PIPE_RING) req = t;
            (*lead_req)[D] = req;
        }
    });
    lap("ring-row reuse");
}

// Awake intervals of dp_pipe.hip's compute waves.  Wave w owns the rows r with (r % 256) / 64 == w; it
// has to run from PG_PIPE_WAKE diagonals before one of its rows enters the band (operand prefetch
// pipeline) until PG_PIPE_RING diagonals after the last one left (so that all its ring columns hold
// -inf again); every wave runs on wide diagonals.  Layout: dp_device.h, PgDevJob::sched.
// (`threads` > 1: the four waves' lists side by side.)
void schedule_waves(const DiagIndex &dx, const std::vector<uint8_t> &cls, std::vector<int> *out, int threads = 1) {
    const int nd = (int)cls.size();
    std::vector<int> lists[4];
    auto one_wave = [&](int w) {
        std::vector<int> next_active(nd + 1);
        auto active = [&](int d) {
            if (cls[d] >= 4) return true;
            const int lo = dx.imin[d], hi = dx.imax[d];
            if (hi < lo) return false;
            const int a = (lo - 64 * w) & 255;                 // lo's position relative to the wave's block
            return a < 64 || lo + (256 - a) <= hi;
        };
        next_active[nd] = 1 << 30;
        for (int d = nd - 1; d >= 0; --d) next_active[d] = active(d) ? d : next_active[d + 1];
        int last_active = -(1 << 30);
        bool awake = false;
        for (int d = 0; d < nd; ++d) {
            if (next_active[d] == d) last_active = d;
            const bool need = next_active[d] - d <= PG_PIPE_WAKE || d - last_active <= PG_PIPE_RING;
            if (need != awake) { lists[w].push_back(d); awake = need; }
        }
        if (awake) lists[w].push_back(nd);
        lists[w].push_back(nd); lists[w].push_back(nd);
    };
    if (threads > 1 && nd >= 16384) {
        std::thread t1([&] { one_wave(1); }), t2([&] { one_wave(2); }), t3([&] { one_wave(3); });
        one_wave(0);
        t1.join(); t2.join(); t3.join();
    } else {
        for (int w = 0; w < 4; ++w) one_wave(w);
    }
    out->assign(4, 0);
    for (int w = 0; w < 4; ++w) {
        (*out)[w] = (int)out->size();
        out->insert(out->end(), lists[w].begin(), lists[w].end());
    }
}

// Row strips (dp_pipe.hip, strip_feeder): a wide job as a chain of banded jobs of PG_STRIP_ROWS rows each.  Per strip the
// diagonal descriptors pg_fill_pipe<true, true> reads (rows of the strip on the diagonal, where its first score lives in the
// PARENT's arrays, class, ring-residency mask, assist hop, ring-reuse rule) and the wave schedule.  Classes as in
// classify_diagonals, with what is different about a strip:
//   * a row stays for the whole sweep, so the rules that send the first / last two rows and columns to the general step would
//     send every diagonal there.  What is special about those is less than the rule says: the gap states extend at the terminal
//     rate in the first / last row (y-gap) and column (x-gap) -- the lanes' own rate for the rows, PG_STRIP_TERM diagonals
//     (C++ step) for the columns --; M(0,0) = 0 meets a free gap-open only in the cells (i,0) / (0,j) whose site has an edge
//     from site 0; site 0 itself has no edge and is computed as a simple site whose predecessors are -inf.  General steps
//     (class 3): diagonals 0 and 1, the diagonals of those cells, sites without edges other than site 0;
//   * operands up to 64 rows above the strip are in the ring (the feeder wave), which covers every operand in reach of the
//     ring (PG_PIPE_REACH - 1 diagonals back); older ones come from L2 through the parent's descriptors.
// Returns false (and leaves *out empty) when some diagonal of some strip holds more multi-edge sites than the assist waves of
// dp_pipe.hip keep in their lanes (64 slots; `max_sites`, default 56): every such diagonal would go through their general
// code, several times slower than the tiled kernel's step.
// big_table (S * S > 256): the compute waves run the C++ step and the assist waves stage EVERY multi-edge cell (and gather every
// cell's model score) with their general code: class 1 = multi-edge cells with every operand in the ring, 2 = one past it; no bound
// on the sites of a diagonal.
bool plan_strips(const pagan_graph *L, const pagan_graph *R, int Lx, int Ly, const RowBand &rb, const DiagIndex &dx,
                 std::vector<StripPlan> *out, int max_sites, int *sites_seen, bool big_table) {
    const int nd = Lx + Ly - 1, REACH = PG_PIPE_REACH, RING = PG_PIPE_RING;
    SiteFeat fl, fr;
    fl.build(L, Lx, true); fr.build(R, Ly, true);
    std::vector<uint8_t> from0L(Lx, 0), from0R(Ly, 0);
    for (int i = 1; i < Lx; ++i) for (int k = L->bwd_off[i]; k < L->bwd_off[i + 1]; ++k) if (L->bwd_src[k] == 0) from0L[i] = 1;
    for (int j = 1; j < Ly; ++j) for (int k = R->bwd_off[j]; k < R->bwd_off[j + 1]; ++k) if (R->bwd_src[k] == 0) from0R[j] = 1;
    // prefix counts: cells (i,0) / (0,j) that meet the free gap-open, sites without edges other than site 0
    std::vector<int> npL(Lx + 1, 0), npR(Ly + 1, 0);
    for (int i = 0; i < Lx; ++i) npL[i + 1] = npL[i] + (i > 0 && L->bwd_off[i + 1] == L->bwd_off[i] ? 1 : 0);
    for (int j = 0; j < Ly; ++j) npR[j + 1] = npR[j] + (j > 0 && R->bwd_off[j + 1] == R->bwd_off[j] ? 1 : 0);
    // columns by span: cols_ge[t] = columns with span >= t (ascending), t = 2 .. REACH-1
    std::vector<std::vector<int>> cols_ge(REACH);
    for (int j = 0; j < Ly; ++j) for (int t = 2; t < REACH && t <= fr.span[j]; ++t) cols_ge[t].push_back(j);
    const int n_strips = (Lx + PG_STRIP_ROWS - 1) / PG_STRIP_ROWS;
    const bool term_cxx = std::getenv("PAGAN_DP_STRIP_TERM") != nullptr;
    // three-edge sites in the lanes (round 5; classify_diagonals has the rules): small model tables only -- the hand-scheduled loop
    const bool three_ok = !big_table && !(std::getenv("PAGAN_DP_THREE") && std::strcmp(std::getenv("PAGAN_DP_THREE"), "0") == 0);
    const std::vector<int> &ne_l = three_ok ? fl.not_easy3 : fl.not_easy, &ne_r = three_ok ? fr.not_easy3 : fr.not_easy;
    std::vector<int> three_cols;
    if (three_ok) for (int j = 0; j < Ly; ++j) if (fr.is_three[j]) three_cols.push_back(j);
    {   // the multi-edge sites a diagonal of a strip holds: the strip's own rows (they stay) + the columns of its window (up to
        // PG_STRIP_ROWS consecutive ones inside the strip's column range)
        int worst = 0;
        for (int k = 0; k < n_strips; ++k) {
            const int r0 = k * PG_STRIP_ROWS, r1 = std::min(r0 + PG_STRIP_ROWS - 1, Lx - 1);
            const int nl = fl.not_simple[r1 + 1] - fl.not_simple[r0];
            const int c0 = rb.lo[r0], c1 = rb.hi[r1];
            int nr = 0;
            for (int c = c0; c <= c1; c += 32) {
                const int e = std::min(c + PG_STRIP_ROWS - 1, c1);
                nr = std::max(nr, fr.not_simple[e + 1] - fr.not_simple[c]);
            }
            worst = std::max(worst, nl + nr);
        }
        if (sites_seen) *sites_seen = worst;
        if (worst > max_sites && !big_table) { out->clear(); return false; }
    }
    out->assign(n_strips, StripPlan());
    for (int k = 0; k < n_strips; ++k) {
        StripPlan &sp = (*out)[k];
        const int r0 = k * PG_STRIP_ROWS, r1 = std::min(r0 + PG_STRIP_ROWS - 1, Lx - 1);
        sp.r0 = r0; sp.r1 = r1;
        sp.feed_wave = k == 0 ? -1 : ((r0 / 64) + 3) & 3;
        // the diagonals on which the strip holds a cell: row + lo[row] and row + hi[row] grow with the row
        int dlo = nd, dhi = -1;
        for (int i = r0; i <= r1; ++i) if (rb.hi[i] >= rb.lo[i]) { dlo = std::min(dlo, i + rb.lo[i]); dhi = std::max(dhi, i + rb.hi[i]); }
        if (dhi < dlo) { dlo = std::min(nd - 1, r0); dhi = dlo; }        // (no cell at all: one empty diagonal keeps the chain of strips whole)
        const int D0 = std::max(0, dlo - 16), D1 = std::min(nd, dhi + 17), m = D1 - D0;
        sp.d0 = D0; sp.d1 = D1;
        std::vector<int> smin(m), smax(m);
        for (int t = 0; t < m; ++t) {
            const int d = D0 + t;
            smin[t] = std::max(r0, dx.imin[d]); smax[t] = std::min(r1, dx.imax[d]);
            // a diagonal without a cell of the strip: the first row stays where it was (it never falls, and a lane whose row
            // fell behind it moves on by 256 rows -- beyond any last row the strip can have), no row is in the band
            if (smax[t] < smin[t]) { smin[t] = t > 0 ? std::min(smin[t - 1], r1) : r0; smin[t] = std::max(smin[t], r0); smax[t] = smin[t] - 1; }
        }
        {   // first column the loader stages: the smallest column of the strip's first diagonals, rounded down to a chunk
            int c0 = Ly;
            for (int t = 0; t < m; ++t) if (smax[t] >= smin[t]) { c0 = D0 + t - smax[t]; break; }
            c0 = std::max(0, std::min(c0, Ly - 1) - 16);
            sp.col_first = c0 & ~63;
        }
        // ---- cells whose operands leave the ring (by age) ----
        std::vector<int> far(m + 1, 0);
        auto mark = [&](int a, int b) { a = std::max(a, D0); b = std::min(b, D1 - 1); if (a <= b) { ++far[a - D0]; --far[b + 1 - D0]; } };
        for (int i = r0; i <= r1; ++i) {
            if (rb.hi[i] < rb.lo[i]) continue;
            const int sl = fl.span[i];
            if (three_ok && fl.is_three[i])         // (classify_diagonals: a cell where two three-edge sites meet stays with the assist waves)
                for (auto it = std::lower_bound(three_cols.begin(), three_cols.end(), rb.lo[i]); it != three_cols.end() && *it <= rb.hi[i]; ++it) mark(i + *it, i + *it);
            if (sl >= REACH - 1) { mark(i + rb.lo[i], i + rb.hi[i]); continue; }
            if (sl < 2) continue;
            const std::vector<int> &cl = cols_ge[REACH - sl];             // span(j) >= REACH - span(i)
            for (auto it = std::lower_bound(cl.begin(), cl.end(), rb.lo[i]); it != cl.end() && *it <= rb.hi[i]; ++it) mark(i + *it, i + *it);
        }
        for (int j : cols_ge[REACH - 1]) {
            // rows of the strip whose band holds column j: hi[] and lo[] are monotone
            int i1 = (int)(std::lower_bound(rb.hi.begin(), rb.hi.end(), j) - rb.hi.begin());
            int i2 = (int)(std::upper_bound(rb.lo.begin(), rb.lo.end(), j) - rb.lo.begin()) - 1;
            i1 = std::max(i1, r0); i2 = std::min(i2, r1);
            if (i1 <= i2) mark(i1 + j, i2 + j);
        }
        // ---- classes ----
        std::vector<uint8_t> cls(m, 0), ring2(m, 0), tbit(m, 0);
        int run = 0;
        for (int t = 0; t < m; ++t) {
            run += far[t];
            const int d = D0 + t, lo = smin[t], hi = smax[t];
            if (hi < lo) { cls[t] = 0; continue; }
            const int jlo = d - hi, jhi = d - lo;
            bool general = d <= 1;
            if (d >= lo && d <= hi && d < Lx && from0L[d]) general = true;                 // cell (d, 0), an edge from site 0
            if (lo == 0 && d < Ly && from0R[d]) general = true;                            // cell (0, d)
            if (npL[hi + 1] - npL[lo] > 0 || npR[jhi + 1] - npR[jlo] > 0) general = true;  // a site without bwd edges (not site 0)
            const bool multi = fl.not_simple[hi + 1] - fl.not_simple[lo] > 0 || fr.not_simple[jhi + 1] - fr.not_simple[jlo] > 0;
            const bool hard = ne_l[hi + 1] - ne_l[lo] > 0 || ne_r[jhi + 1] - ne_r[jlo] > 0;
            uint8_t c;
            if (general) c = 3;
            else if (run > 0) c = 2;
            else if (multi) c = (hard && !big_table) ? 2 : 1;
            else c = 0;
            ring2[t] = c == 2 && run == 0;
            tbit[t] = three_ok && c == 1 && (fl.three[hi + 1] - fl.three[lo] > 0 || fr.three[jhi + 1] - fr.three[jlo] > 0);
            const bool term = (d >= lo && d <= hi) || (d - (Ly - 1) >= lo && d - (Ly - 1) <= hi);      // a cell of column 0 / column Ly-1
            // (the strip's assembly loop picks the x-gap rate per lane: such a diagonal needs no path of its own; PAGAN_DP_STRIP_TERM=1
            //  sends it to the C++ step all the same -- A/B switch)
            if (c <= 2 && term && term_cxx) c |= PG_STRIP_TERM;
            cls[t] = c;
        }
        // ---- ring reuse (classify_diagonals has the reasoning) ----
        std::vector<int> need(m, REACH - 1);
        {
            std::vector<int> rowsL;
            for (int i = r0; i <= r1; ++i) if (fl.span_ring[i] >= 2) rowsL.push_back(i);
            size_t la = 0, lb = 0;
            for (int t = 0; t < m; ++t) {
                const int d = D0 + t, lo = smin[t], hi = smax[t];
                if (hi < lo || (cls[t] & 7) > 2) continue;
                while (lb < rowsL.size() && rowsL[lb] <= hi) ++lb;
                while (la < lb && rowsL[la] < lo) ++la;
                int mx = 2;
                for (size_t q = la; q < lb; ++q) {
                    const int i = rowsL[q];
                    if (fl.span_ring[i] > (i & 63)) mx = std::max(mx, fl.span_ring[i] + fr.span_ring[d - i]);
                }
                for (int i = (lo + 63) & ~63; i <= hi; i += 64) mx = std::max(mx, fl.span_ring[i] + fr.span_ring[d - i]);
                need[t] = std::min(mx, REACH - 1);
            }
        }
        std::vector<int> lead(m, -1);
        for (int D = D0 + RING; D < D1; ++D) {
            int req = -1;
            for (int t = D - RING + 1; t <= D - RING + REACH - 1 && t < D1; ++t)
                if (t >= D0 && t - need[t - D0] <= D - RING) req = t;
            lead[D - D0] = req;
        }
        // ---- the wave schedule (schedule_waves over the strip's own diagonals, shifted) ----
        {
            DiagIndex sdx;
            sdx.imin = smin; sdx.imax = smax;
            std::vector<uint8_t> c7(m);
            for (int t = 0; t < m; ++t) c7[t] = cls[t] & 7;
            schedule_waves(sdx, c7, &sp.sched);
            for (size_t q = 4; q < sp.sched.size(); ++q) sp.sched[q] += D0;
        }
        // ---- descriptors ----
        sp.psc.assign(8 * ((size_t)m + 1), 0);
        std::vector<int> hop(m, 0);
        for (int t = m; t-- > 0;) {
            const int nx = t + PG_PIPE_ASSIST;
            if (nx >= m) { hop[t] = 4095; continue; }
            const bool work = (cls[nx] & 7) == 2 || (big_table && (cls[nx] & 7) <= 1);     // (large tables: every interior diagonal's model scores)
            hop[t] = work ? 1 : std::min(4095, hop[nx] + 1);
        }
        unsigned mask = 0;
        for (int t = 0; t < m; ++t) {
            const int d = D0 + t;
            int *pk = sp.psc.data() + 8 * (size_t)t;
            pk[0] = smin[t]; pk[1] = smax[t];
            const long long boff = 24 * (dx.doff[d] + (smin[t] - dx.imin[d]));
            pk[2] = (int)(boff & 0xffffffffLL); pk[3] = (int)(boff >> 32);
            mask = t >= 1 ? (((mask << 1) | 2u) & (((1u << REACH) - 1u) & ~1u)) : 0u;
            // bit 4: large tables -- the next step is hot too; small tables -- a class 2 diagonal with every operand in the ring
            const unsigned pair = big_table ? (t + 1 < m && (cls[t + 1] & 7) <= 2 ? 1u : 0u) : (ring2[t] ? 1u : 0u);
            pk[4] = (int)(cls[t] | (pair << 4) | (mask << 5) | ((unsigned)tbit[t] << 19) | ((unsigned)hop[t] << 20));     // (bit 19: the lanes' third pass, as in a banded job's descriptors)
            pk[5] = 0; pk[6] = 0;
            pk[7] = lead[t];
        }
    }
    return true;
}

// Tiles of dp_tiles.hip: PG_TILE x PG_TILE squares of the matrix that the band touches.  The band is monotone,
// so the columns of a block of rows run from the first row's lower bound to the last row's upper bound.
void list_tiles(int Lx, const RowBand &rb, std::vector<int> *out) {
    out->clear();
    for (int a = 0; a * PG_TILE < Lx; ++a) {
        const int i1 = std::min(Lx, (a + 1) * PG_TILE);
        int cmin = 1 << 30, cmax = -1;
        for (int i = a * PG_TILE; i < i1; ++i)
            if (rb.hi[i] >= rb.lo[i]) { cmin = std::min(cmin, rb.lo[i]); cmax = std::max(cmax, rb.hi[i]); }
        for (int b = cmin / PG_TILE; cmax >= 0 && b <= cmax / PG_TILE; ++b) { out->push_back(a); out->push_back(b); }
    }
}

// dp_tiles.hip stages the bwd edges of a tile's 64 rows and 64 columns in LDS windows of PG_TILE_EDGES entries
// A job's tiles (tile row, tile column pairs) form a staircase: every tile row a contiguous run of columns, first and last
// column never falling from one row to the next, no empty row between two rows, consecutive rows touching.  Then waiting
// for a tile's three neighbours orders it behind every tile (a',b') <= (a,b) (dp_tiles.hip, pg_fill_tiles_flow).
bool tiles_staircase(const std::vector<int> &tl) {
    std::vector<std::pair<int, int>> span;             // per tile row: first, last column
    std::vector<int> count;
    for (size_t q = 0; q < tl.size(); q += 2) {
        const int a = tl[q], bb = tl[q + 1];
        if ((int)span.size() <= a) { span.resize(a + 1, {1 << 30, -1}); count.resize(a + 1, 0); }
        span[a].first = std::min(span[a].first, bb); span[a].second = std::max(span[a].second, bb);
        ++count[a];
    }
    int prev = -1;
    for (int a = 0; a < (int)span.size(); ++a) {
        if (count[a] == 0) { if (prev >= 0) return false; continue; }     // (rows before the first tile row are fine)
        if (count[a] != span[a].second - span[a].first + 1) return false;
        if (prev >= 0 && (prev != a - 1 || span[a].first < span[prev].first || span[a].second < span[prev].second ||
                          span[a].first > span[prev].second + 1)) return false;
        prev = a;
    }
    return true;
}

bool edges_fit_tiles(const pagan_graph *g, int n) {
    for (int a = 0; a < n; a += PG_TILE)
        if (g->bwd_off[std::min(n, a + PG_TILE)] - g->bwd_off[a] > PG_TILE_EDGES) return false;
    return true;
}

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

struct Arena {
    char *dev = nullptr;
    size_t size = 0;         // bytes the batch uses
    size_t cap = 0;          // bytes allocated (an arena taken from the pool may be larger)
};

// Device arenas are reused by the next batch on the same device: hipFree of a few GB costs 10-30 ms, and a level
// of a tree walk is followed by the next.  At most two idle arenas per device; pagan_dp_release_cache() frees them.
struct ArenaPool {
    struct Slot { char *p; size_t cap; int device; };
    std::mutex m;
    std::vector<Slot> idle;
    char *take(int device, size_t n, size_t *cap) {
        std::lock_guard<std::mutex> g(m);
        int best = -1;
        for (size_t k = 0; k < idle.size(); ++k)
            if (idle[k].device == device && idle[k].cap >= n && (best < 0 || idle[k].cap < idle[best].cap)) best = (int)k;
        if (best < 0) return nullptr;
        char *p = idle[best].p;
        *cap = idle[best].cap;
        idle.erase(idle.begin() + best);
        return p;
    }
    void give(int device, char *p, size_t cap) {
        std::vector<char *> drop;
        {
            std::lock_guard<std::mutex> g(m);
            idle.push_back({p, cap, device});
            for (;;) {
                int count = 0, smallest = -1;
                for (size_t k = 0; k < idle.size(); ++k)
                    if (idle[k].device == device) { ++count; if (smallest < 0 || idle[k].cap < idle[smallest].cap) smallest = (int)k; }
                if (count <= 2) break;
                drop.push_back(idle[smallest].p);
                idle.erase(idle.begin() + smallest);
            }
        }
        for (char *q : drop) (void)hipFree(q);
    }
    // frees the idle arenas of one device (-1: all)
    void clear(int device) {
        std::vector<char *> drop;
        {
            std::lock_guard<std::mutex> g(m);
            for (size_t k = 0; k < idle.size();)
                if (device < 0 || idle[k].device == device) { drop.push_back(idle[k].p); idle.erase(idle.begin() + k); } else ++k;
        }
        for (char *q : drop) (void)hipFree(q);
    }
    size_t idle_bytes(int device) {
        std::lock_guard<std::mutex> g(m);
        size_t n = 0;
        for (const Slot &s : idle) if (s.device == device) n += s.cap;
        return n;
    }
};
ArenaPool arena_pool;

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
struct GpuObjPool {
    std::mutex m;
    std::vector<std::pair<int, GpuObjs>> idle;
    bool take(int device, GpuObjs *o) {
        std::lock_guard<std::mutex> g(m);
        for (size_t k = 0; k < idle.size(); ++k)
            if (idle[k].first == device) { *o = idle[k].second; idle.erase(idle.begin() + k); return true; }
        return false;
    }
    void give(int device, const GpuObjs &o) {
        GpuObjs drop;
        bool dropping = false;
        {
            std::lock_guard<std::mutex> g(m);
            int have = 0;
            for (auto &e : idle) have += e.first == device;
            if (have >= 4) { drop = o; dropping = true; }
            else idle.emplace_back(device, o);
        }
        if (dropping) drop.destroy();
    }
    void release() {
        std::vector<std::pair<int, GpuObjs>> all;
        { std::lock_guard<std::mutex> g(m); all.swap(idle); }
        for (auto &e : all) { (void)hipSetDevice(e.first); e.second.destroy(); }
    }
};
GpuObjPool gpu_pool;

} // namespace

// ---- dead sites ----------------------------------------------------------------------------------------------------
// A site without bwd edges (other than the start site) -- or with bwd edges from such sites only -- has no live
// predecessor: every cell of its row / column is -inf in all three states, nothing can leave it, and no path visits it (the path SKIPS it: insert_preexisting_gap,
// viterbi_alignment.h:146-193, restated in replay()).  High in a deep tree such sites are many (root of 512 x 10 kb: 44 %
// of each sequence), so the alignment is run on the COMPACTED graphs -- dead sites removed, the edges that start at one
// dropped (their candidates are -inf), the band re-indexed -- and the device's path is mapped back to the caller's site
// numbers and edge-list positions before replay() turns it into columns and used edges.  Scores, path and used edges are
// the ones of the full matrices; `cells` stays the caller's count.  PAGAN_DP_COMPACT=0 switches it off.
struct CompactSide {
    std::vector<int> keep;       // compacted site -> caller's site
    std::vector<int> state, off, src, eid, slot;   // compacted graph arrays; slot: position of the edge in the caller's list of its site
    std::vector<float> w;
    pagan_graph g;
    int dead = 0;
    void build(const pagan_graph *o) {
        const int n = o->n_sites;
        std::vector<int> newidx(n, -1);
        keep.clear();
        for (int s_ = 0; s_ < n; ++s_) {
            // dead: no bwd edge, or (bwd edges point to earlier sites, so one ascending pass sees the whole cascade) none
            // from a site that is alive
            // (the last site before the end site stays whatever it is: the terminal-gap rules, VA:875-879 and its X twin,
            // name the LAST row / column of the matrix, and that must be the same site in both numberings)
            bool is_dead = s_ != 0 && s_ < n - 2;
            for (int e = o->bwd_off[s_]; is_dead && e < o->bwd_off[s_ + 1]; ++e) {
                const int from = o->bwd_src[e];
                if (from >= s_ || (from >= 0 && newidx[from] >= 0)) is_dead = false;      // (an edge that is not backward: keep the site)
            }
            if (is_dead) { ++dead; continue; }
            newidx[s_] = (int)keep.size();
            keep.push_back(s_);
        }
        const int m = (int)keep.size();
        state.resize(m); off.assign(m + 1, 0);
        src.clear(); eid.clear(); slot.clear(); w.clear();
        for (int t = 0; t < m; ++t) {
            const int s_ = keep[t];
            state[t] = o->state[s_];
            off[t] = (int)src.size();
            for (int e = o->bwd_off[s_]; e < o->bwd_off[s_ + 1]; ++e) {
                const int from = o->bwd_src[e];
                if (from < 0 || from >= n || newidx[from] < 0) continue;      // (a bad index is check_graph's to report)
                src.push_back(newidx[from]); w.push_back(o->bwd_logw[e]); eid.push_back(o->bwd_eid[e]); slot.push_back(e - o->bwd_off[s_]);
            }
        }
        off[m] = (int)src.size();
        g.n_sites = m; g.n_edges = o->n_edges; g.state = state.data(); g.bwd_off = off.data();
        g.bwd_src = src.data(); g.bwd_logw = w.data(); g.bwd_eid = eid.data();
    }
};
struct CompactJob {
    bool on = false;
    const pagan_graph *L0 = nullptr, *R0 = nullptr;   // the caller's graphs
    int64_t cells0 = 0;                               // the caller's in-band cells
    CompactSide l, r;
    std::vector<int> up, lo;
    pagan_band band;
};

// The caller's band over the compacted matrices: row t is the caller's row l.keep[t]; its interval keeps the first / last
// kept column inside the caller's interval (empty where none is).  rb0: the caller's band, clamped (RowBand).
void compact_band(const RowBand &rb0, const CompactSide &l, const CompactSide &r, int nr, std::vector<int> *up, std::vector<int> *lo) {
    // columns: the right graph's sites below its end site; kept columns before column c: before[c]
    std::vector<int> before(nr, 0);
    {
        size_t q = 0;
        for (int c = 0; c < nr; ++c) {
            before[c] = (int)q;
            if (q < r.keep.size() && r.keep[q] == c) ++q;
        }
    }
    const int rows = (int)l.keep.size() - 1;                    // kept sites below the left end site
    up->resize(rows); lo->resize(rows);
    for (int t = 0; t < rows; ++t) {
        const int i = l.keep[t];
        const int a = rb0.lo[i], z = rb0.hi[i];                  // clamped to the matrix by RowBand
        (*up)[t] = before[a];                                     // first kept column >= a
        (*lo)[t] = (z + 1 < nr ? before[z + 1] : before[nr - 1] + 1) - 1;      // last kept column <= z
    }
}

// (PAGAN_DP_CANARY: guard words behind every region of the arena -- Carver, further down)
#define PG_CANARY_BYTES 64
#define PG_CANARY_WORD 0x5ca1ab1eu
// pagan_dp_align_batch's third attempt (below): the batch is planned again with every wide job on the tiled kernel
static thread_local bool tl_no_strips = false;
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
    int *d_which = nullptr;      // [n]: ring-kernel jobs first, then the ones of the HBM wavefront kernel
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
    hipStream_t pooled_stream2 = nullptr;                       // (owned through the pool whether this batch forks or not)
    hipEvent_t pooled_fork = nullptr, pooled_join = nullptr;
    hipStream_t stream2 = nullptr;   // the tile launches, when the batch also has jobs of the other kernels
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    int n_ring_small = 0;        // ring jobs whose model table fits the LDS cache (listed first)
    bool use_pipe = true;        // LDS-staged jobs run pg_fill_pipe (default) or the older pg_fill_ring
    int bp_pass = 1;             // pg_fill_pipe's jobs: 1 back-pointers by pg_backptr after the fill (its hot loop stores scores only),
                                 // 2 (PAGAN_DP_BP=verify, diagnostic builds that still write them in the fill) pg_backptr compares
    int max_bound = 0;           // largest traceback boundary count of any job
    int max_entries = 0;         // most traceback table entries of any job (tb[n_bound + 1])
    size_t follow_begin = 0, follow_bytes = 0;     // PgDevJob::follow / bp_done of the banded jobs, one block zeroed per launch
    hipStream_t stream = nullptr;
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    // PAGAN_DP_CANARY=1: guard words behind every region of the arena (Carver)
    std::vector<size_t> guards;
    size_t *d_guards = nullptr;
    int *d_canary = nullptr;                     // [0] guards found changed by the last run, [1] the first of them
    bool strip_xcd_failure = false;              // pagan_batch_fetch: a strip found the strip above on another XCD in the launch of the strips alone, too
    unsigned canary_word = PG_CANARY_WORD;       // (PAGAN_DP_CANARY=0x...: another pattern -- what a read past a region's end then sees)
    // per-kernel brackets inside the fill (pagan_batch_last_ms_detail): 0/1 around the banded kernel, 2 behind pg_backptr,
    // 3/4 around the tiled kernel (on its own stream when the batch also has banded jobs), 5 behind the HBM wavefront
    hipEvent_t evk[7] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};      // (6: behind the tiled jobs' pg_backptr)
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

int validate_job(const pagan_job &jb, HostJob *hj, RowBand *rb, bool use_pipe, int threads = 1) {
    if (!jb.left || !jb.right || !jb.model) return PAGAN_E_ARG;
    int rc;
    // (PAGAN_DP_PLAN_PROFILE: milliseconds per phase of the plan of one job, on stderr)
    static const bool prof = std::getenv("PAGAN_DP_PLAN_PROFILE") != nullptr;
    auto now = [] { return std::chrono::steady_clock::now(); };
    auto t_last = now();
    auto lap = [&](const char *what) {
        if (!prof) return;
        const auto t = now();
        std::fprintf(stderr, "pagan_dp: plan %s %.2f ms\n", what, std::chrono::duration<double, std::milli>(t - t_last).count());
        t_last = t;
    };
    if ((rc = check_graph(jb.left)) != PAGAN_OK) return rc;
    if ((rc = check_graph(jb.right)) != PAGAN_OK) return rc;
    const pagan_model *m = jb.model;
    if (m->n_states <= 0 || !m->log_score) return PAGAN_E_MODEL;
    hj->L = jb.left; hj->R = jb.right;
    hj->Lx = jb.left->n_sites - 1; hj->Ly = jb.right->n_sites - 1;
    for (int s = 1; s < hj->Lx; ++s)
        if (jb.left->state[s] < 0 || jb.left->state[s] >= m->n_states) return PAGAN_E_MODEL;
    for (int s = 1; s < hj->Ly; ++s)
        if (jb.right->state[s] < 0 || jb.right->state[s] >= m->n_states) return PAGAN_E_MODEL;
    lap("checks");
    if ((rc = rb->build(hj->Lx, hj->Ly, jb.band)) != PAGAN_OK) return rc;
    lap("row band");
    hj->dx.build(hj->Lx, hj->Ly, *rb);
    if (hj->dx.cells != rb->cells()) return PAGAN_E_INTERNAL;
    lap("diagonal index");
    // The LDS-staged kernel suits banded work: most diagonals narrow.  A full matrix (or a band that is
    // mostly wider than the ring) goes to the multi-wave HBM wavefront instead.
    // traceback boundaries k = 1..K at diagonals k*PG_SEG (<= nd-1): 3 table entries per cell of
    // the diagonals k*PG_SEG and k*PG_SEG-1
    {
        const int nd = hj->Lx + hj->Ly - 1;
        hj->n_bound = (nd - 1) / PG_SEG;
        hj->tb.assign(hj->n_bound + 2, 0);
        int run = 0, widest = 0;
        for (int k = 1; k <= hj->n_bound; ++k) {
            hj->tb[k] = run;
            const int D = k * PG_SEG;
            const int wa = hj->dx.imax[D] - hj->dx.imin[D] + 1, wb = hj->dx.imax[D - 1] - hj->dx.imin[D - 1] + 1;
            const int e = 3 * ((wa > 0 ? wa : 0) + (wb > 0 ? wb : 0));
            run += e;
            widest = std::max(widest, e);
        }
        hj->tb[hj->n_bound + 1] = run;
        // The segmented traceback chases from EVERY cell of every boundary: 2 x cells chase steps of speculative work, dealt
        // one table entry per thread over the whole chip (pg_trace_spec), against one lane's serial chase of Lx + Ly
        // dependent reads at 0.3 - 1.4 us each (pg_trace_compose with no boundaries).  Measured (round 3, one thread per
        // entry): 16 x 2 kb full matrices 2.0 -> 0.8 ms per level, the full-matrix top levels of 512 x 10 kb 13 -> 7 ms;
        // only very short paths, or matrices ten thousand cells wide on average, are left to the serial chase.
        const long long speculative = (long long)run / 3 * PG_SEG, serial = (long long)hj->Lx + hj->Ly;
        (void)widest;
        if (serial < 2000 || speculative > 20000 * serial) {
            hj->n_bound = 0;
            hj->tb.assign(2, 0);
        }
    }
    bool narrow = hj->dx.cells <= (long long)PG_RING_MAX_WIDTH * hj->dx.imin.size() / 2;
    // The LDS kernels take maxima with v_max_f64, which returns +0 for (+0, -0) in either order where the
    // reference's compare keeps the incumbent's sign: a job with a negative zero among its parameters
    // runs on the HBM wavefront kernel, which compares.
    const bool neg0 = has_negative_zero(jb);
    if (neg0) narrow = false;
    if (const char *f = std::getenv("PAGAN_DP_FILL")) if (std::strcmp(f, "tiles") == 0) narrow = false;   // A/B switch
    if (use_pipe) {
        hj->ring_ok = narrow && edges_fit_ring(jb.left, hj->Lx, PG_PIPE_EDGE_CAP, PG_PIPE_SITE_EDGES) &&
                      edges_fit_ring(jb.right, hj->Ly, PG_PIPE_EDGE_CAP, PG_PIPE_SITE_EDGES);
        if (hj->ring_ok) {
            lap("boundaries, edge windows");
            FarPlan fp;
            classify_diagonals(jb.left, jb.right, hj->Lx, hj->Ly, *rb, hj->dx, jb.model->n_states * jb.model->n_states <= 256,
                               &hj->cls, &hj->lead_req, &hj->ring2, threads, &fp);
            if (fp.n_served > 0) { hj->hfL.swap(fp.hfL); hj->hfR.swap(fp.hfR); hj->hbit.swap(fp.hbit); }
            if (std::find(fp.tbit.begin(), fp.tbit.end(), (uint8_t)1) != fp.tbit.end()) hj->tbit.swap(fp.tbit);
            lap("classify_diagonals");
            schedule_waves(hj->dx, hj->cls, &hj->sched, threads);
            lap("schedule_waves");
        }
    } else {
        hj->ring_ok = narrow && edges_fit_ring(jb.left, hj->Lx) && edges_fit_ring(jb.right, hj->Ly);
    }
    if (!hj->ring_ok && !neg0 && edges_fit_tiles(jb.left, hj->Lx) && edges_fit_tiles(jb.right, hj->Ly))
        list_tiles(hj->Lx, *rb, &hj->tiles);
    // Row strips on the banded kernel (dp_pipe.hip, strip_feeder): a wide job whose model table fits LDS and whose edge lists
    // fit the kernel's windows, unless a diagonal of a strip would hold more multi-edge sites than the kernel's assist waves
    // keep in their lanes (plan_strips).  PAGAN_DP_WIDE=tiles keeps every wide job on the tiled kernel (A/B switch).
    {
        const char *we = std::getenv("PAGAN_DP_WIDE");
        const bool want = (!we || std::strcmp(we, "strips") == 0) && !tl_no_strips;
        // Models whose table does not fit LDS (S > 16) run as strips only on request (PAGAN_DP_STRIP_STATES = the largest model that
        // does): correct (tests/test_strips_gpu.py) and slower than the tiles from the third level of a tree on -- the assist
        // waves gather a model score for every cell and stage every multi-edge cell with their general code (cfg3: 23.4 -> 57.8 ms).
        int max_states = 16;
        if (const char *e = std::getenv("PAGAN_DP_STRIP_STATES")) max_states = std::atoi(e);
        if (want && use_pipe && !hj->ring_ok && !neg0 && !hj->tiles.empty() && jb.model->n_states <= max_states &&
            hj->Lx >= 2 && hj->Ly >= 2 &&
            edges_fit_ring(jb.left, hj->Lx, PG_PIPE_EDGE_CAP, PG_PIPE_SITE_EDGES) && edges_fit_ring(jb.right, hj->Ly, PG_PIPE_EDGE_CAP, PG_PIPE_SITE_EDGES))
        {
            int max_sites = 56, seen = 0;
            if (const char *e = std::getenv("PAGAN_DP_STRIP_SITES")) max_sites = std::atoi(e);
            const bool ok = plan_strips(jb.left, jb.right, hj->Lx, hj->Ly, *rb, hj->dx, &hj->strips, max_sites, &seen,
                                        jb.model->n_states * jb.model->n_states > 256);
            if (std::getenv("PAGAN_DP_VERBOSE"))
                std::fprintf(stderr, "pagan_dp: wide job %d x %d: at most %d multi-edge sites on a strip's diagonal: %s\n", hj->Lx, hj->Ly, seen,
                             ok ? "row strips" : "tiles");
        }
    }
    return PAGAN_OK;
}

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
        cur = align_up(cur + sizeof(T) * (count ? count : 1));
        if (guards) { guards->push_back(cur); cur = align_up(cur + PG_CANARY_BYTES); }
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

int launch_fill(pagan_batch *b) {
    // Full-matrix score check (PG_FLAG_SCORE_CHECK; dp_kernels.hip, pg_backptr): whoever writes a cell's back-pointers has just
    // re-evaluated its three scores from the stored scores of its predecessors -- comparing them with the cell's own stored
    // scores proves the recurrence at every cell.  On for the banded kernel's jobs (the follower workgroups do it on compute
    // units the fill leaves idle) and for batches with row strips (scores cross workgroups on a landing rule there);
    // PAGAN_DP_SCORE_CHECK=0 switches it off, =all extends it to every tiled job's pass.
    unsigned chk_banded = PG_FLAG_SCORE_CHECK, chk_wide = b->n_striped > 0 ? PG_FLAG_SCORE_CHECK : 0u;
    if (const char *e = std::getenv("PAGAN_DP_SCORE_CHECK")) {
        if (std::strcmp(e, "0") == 0) { chk_banded = 0; chk_wide = 0; }
        else if (std::strcmp(e, "all") == 0) chk_wide = PG_FLAG_SCORE_CHECK;
    }
    const unsigned spread = b->strips_spread ? PG_FLAG_STRIPS_SPREAD : 0u;
    hipStream_t tile_stream = nullptr;
    static std::atomic<int> n_cu_dev[64];
    bool ev3_recorded = false;
    if (b->n_striped > 0 && b->strips_alone) {
        // (workgroup g of a dispatch runs on XCD g % 8 -- what puts a job's strips on one XCD -- when nothing else is being
        //  dispatched beside it: first on the batch's stream, everything else behind it)
        HIP_TRY(hipMemsetAsync(b->arena.dev + b->sfollow_begin, 0, b->sfollow_bytes, b->stream));
        if (b->strip_grid > 0)
            hipLaunchKernelGGL((pg_fill_pipe<true, true>), dim3(b->strip_grid), dim3(pg_pipe_block()), 0, b->stream,
                               b->d_jobs, b->d_swhich, ((b->flags & 0x400u) ? b->flags : (b->flags & ~0x800u)) | spread, b->strip_grid);
        if (b->strip_grid_big > 0)
            hipLaunchKernelGGL((pg_fill_pipe<false, true>), dim3(b->strip_grid_big), dim3(pg_pipe_block()), 0, b->stream,
                               b->d_jobs, b->d_swhich + b->strip_grid, ((b->flags & 0x400u) ? b->flags : (b->flags & ~0x800u)) | spread, b->strip_grid_big);
    }
    if (b->n_striped > 0 && b->tile_off.size() <= 1) {
        // (the strips' stream: beside the banded kernels, as the tiles')
        hipStream_t st = b->stream;
        if (b->stream2) {
            HIP_TRY(hipEventRecord(b->ev_fork, b->stream));
            HIP_TRY(hipStreamWaitEvent(b->stream2, b->ev_fork, 0));
            st = b->stream2;
        }
        tile_stream = st;
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
        hipStream_t st = b->stream;
        if (b->stream2) {
            HIP_TRY(hipEventRecord(b->ev_fork, b->stream));
            HIP_TRY(hipStreamWaitEvent(b->stream2, b->ev_fork, 0));
            st = b->stream2;
        }
        tile_stream = st;
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
        HIP_TRY(hipEventRecord(b->evk[0], b->stream)); b->evk_set[0] = true;
        if (b->use_pipe) {
            // Follower workgroups behind the fill's (dp_pipe.hip, pipe_follower): they write the back-pointers of the diagonals
            // whose scores have landed while the fill goes on, on compute units the banded fill leaves idle.  Workgroup g of
            // a dispatch runs on XCD g % 8 and a follower serves the fill workgroups of its own XCD (it shares their L2), so
            // eight followers per round of eight jobs are the unit; what they do not get to is left to pg_backptr below.
            bool follow = b->bp_pass == 1 && b->follow_bytes > 0 && !b->no_follow;
            if (const char *f = std::getenv("PAGAN_DP_FOLLOW")) follow = follow && std::strcmp(f, "0") != 0;
            if (b->follow_bytes > 0) HIP_TRY(hipMemsetAsync(b->arena.dev + b->follow_begin, 0, b->follow_bytes, b->stream));
            // (a dispatch of more than 32 jobs fills the chip by itself: pg_backptr afterwards, on every unit, is the faster pass)
            auto followers = [&](int n_fill) { return follow && n_fill <= 32 ? std::min(96, 48 * ((n_fill + 7) / 8)) : 0; };
            if (n_small > 0)
                hipLaunchKernelGGL((pg_fill_pipe<true, false>), dim3(n_small + followers(n_small)), dim3(pg_pipe_block()), 0 /* its LDS is static */, b->stream,
                                   b->d_jobs, b->d_which, b->flags | chk_banded, n_small);
            if (n_big > 0)
                hipLaunchKernelGGL((pg_fill_pipe<false, false>), dim3(n_big + followers(n_big)), dim3(pg_pipe_block()), 0, b->stream,
                                   b->d_jobs, b->d_which + n_small, b->flags | chk_banded, n_big);
            HIP_TRY(hipEventRecord(b->evk[1], b->stream)); b->evk_set[1] = true;
            if (b->bp_pass) {
                int max_nd = 1, max_w = 1;
                for (int k = 0; k < b->n; ++k) if (b->jobs[k].ring_ok) { max_nd = std::max(max_nd, b->dj[k].nd); max_w = std::max(max_w, b->jobs[k].dx.max_width); }
                const int zc = (max_w + PG_BP_CELLS - 1) / PG_BP_CELLS, dpb = bp_diags_per_block(max_nd, b->n_ring * zc);
                hipLaunchKernelGGL(pg_backptr, dim3((max_nd + dpb - 1) / dpb, b->n_ring, zc), dim3(256), 0, b->stream,
                                   b->d_jobs, b->d_which, (b->flags & 0xffu) | (b->bp_pass == 2 ? 0x100u : chk_banded), dpb);
                HIP_TRY(hipEventRecord(b->evk[2], b->stream)); b->evk_set[2] = true;
            }
        } else {
            b->evk_set[1] = false;
            if (n_small > 0)
                hipLaunchKernelGGL(pg_fill_ring<true>, dim3(n_small), dim3(576), pg_ring_lds_bytes(), b->stream,
                                   b->d_jobs, b->d_which, b->flags);
            if (n_big > 0)
                hipLaunchKernelGGL(pg_fill_ring<false>, dim3(n_big), dim3(576), pg_ring_lds_bytes(), b->stream,
                                   b->d_jobs, b->d_which + n_small, b->flags);
        }
    }
    if (b->n_wide > 0) {
        dim3 grid(b->n_wide);
        const int *which = b->d_which + b->n_ring;
        switch (b->block) {
        case 64: hipLaunchKernelGGL(pg_fill_wavefront<64>, grid, dim3(64), 0, b->stream, b->d_jobs, which, b->flags); break;
        case 256: hipLaunchKernelGGL(pg_fill_wavefront<256>, grid, dim3(256), 0, b->stream, b->d_jobs, which, b->flags); break;
        default: hipLaunchKernelGGL(pg_fill_wavefront<1024>, grid, dim3(1024), 0, b->stream, b->d_jobs, which, b->flags); break;
        }
        HIP_TRY(hipEventRecord(b->evk[5], b->stream)); b->evk_set[5] = true;
    }
    if (b->n_striped > 0 && !b->strips_alone) {
        // row strips of the wide jobs on the banded kernel: one workgroup per strip, a job's strips on one XCD
        HIP_TRY(hipEventRecord(b->evk[3], tile_stream)); b->evk_set[3] = true; ev3_recorded = true;
        HIP_TRY(hipMemsetAsync(b->arena.dev + b->sfollow_begin, 0, b->sfollow_bytes, tile_stream));
        if (b->strip_grid > 0)
            hipLaunchKernelGGL((pg_fill_pipe<true, true>), dim3(b->strip_grid), dim3(pg_pipe_block()), 0, tile_stream,
                               b->d_jobs, b->d_swhich, b->flags | spread, b->strip_grid);
        if (b->strip_grid_big > 0)
            hipLaunchKernelGGL((pg_fill_pipe<false, true>), dim3(b->strip_grid_big), dim3(pg_pipe_block()), 0, tile_stream,
                               b->d_jobs, b->d_swhich + b->strip_grid, b->flags | spread, b->strip_grid_big);
    }
    if (b->tile_off.size() > 1) {
        // after the banded kernels: their workgroups get compute units first; the persistent waves below hold theirs
        hipStream_t st = tile_stream;
        if (!ev3_recorded) { HIP_TRY(hipEventRecord(b->evk[3], st)); b->evk_set[3] = true; }
        if (b->tiles_flow) {
            // one persistent wave per compute unit (a tile fills the LDS) drains the batch's tiles in dependency order
            const int n_tiles = b->tile_off.back(), n_diag = (int)b->tile_off.size() - 1;
            // (last argument) tiles run 80 steps behind their neighbours unless the batch has so many tiles per anti-diagonal
            // that the compute units are the bound either way (measured on cfg5: 575 per diagonal 65 -> 56 ms without the lag,
            // 320 per diagonal 46 -> 48 ms: the switch sits at 1.75 x the number of compute units)
            // no more waves than can have a tile to work on: the tiles of two anti-diagonals (a tile runs 80 steps behind
            // its neighbours) -- a persistent wave holds its compute unit's LDS, which the batch's banded jobs need too
            int widest = 1;
            for (int t = 0; t < n_diag; ++t) widest = std::max(widest, b->tile_off[t + 1] - b->tile_off[t]);
            const int waves = std::min({n_tiles, n_cu_dev[b->device & 63].load(), 2 * widest + 8});
            HIP_TRY(hipMemsetAsync(b->d_flow, 0, sizeof(int) * b->flow_ints, st));
            hipLaunchKernelGGL(pg_fill_tiles_flow, dim3(waves), dim3(64), pg_tiles_lds_bytes(),
                               st, b->d_jobs, b->d_tiles, n_tiles, n_diag, b->d_flow, b->flags,
                               b->tiles_water ? 1 : (4ll * n_tiles >= 7ll * n_cu_dev[b->device & 63].load() * n_diag || b->tiles_nolag ? 2 :
                                                      (2ll * n_tiles < (long long)n_cu_dev[b->device & 63].load() * n_diag ? 3 : 0)));
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
        HIP_TRY(hipEventRecord(b->evk[4], tile_stream)); b->evk_set[4] = true;
        // the tiled fill (and the strips) store scores only: their jobs' back-pointers by the pass, behind them on the same stream
        if (b->n_tiled > 0) {
            int max_nd = 1, max_w = 1;
            for (int k = 0; k < b->n; ++k) if (!b->jobs[k].ring_ok && (!b->jobs[k].tiles.empty() || !b->jobs[k].strips.empty())) { max_nd = std::max(max_nd, b->dj[k].nd); max_w = std::max(max_w, b->jobs[k].dx.max_width); }
            const int zc = (max_w + PG_BP_CELLS - 1) / PG_BP_CELLS, dpb = bp_diags_per_block(max_nd, b->n_tiled * zc);
            hipLaunchKernelGGL(pg_backptr, dim3((max_nd + dpb - 1) / dpb, b->n_tiled, zc), dim3(256), 0, tile_stream,
                               b->d_jobs, b->d_which + b->n_ring + b->n_wide, (b->flags & 0xffu) | chk_wide, dpb);
            HIP_TRY(hipEventRecord(b->evk[6], tile_stream)); b->evk_set[6] = true;
        }
    }
    if ((b->tile_off.size() > 1 || b->n_striped > 0) && b->stream2) {
        HIP_TRY(hipEventRecord(b->ev_join, b->stream2));
        HIP_TRY(hipStreamWaitEvent(b->stream, b->ev_join, 0));
    }
    HIP_TRY(hipGetLastError());
    return PAGAN_OK;
}

// Host side of backtrack_new_path (VA:1038-1189): the device reports the visited cells
// end -> start; this re-inserts the skipped child sites (insert_preexisting_gap,
// viterbi_alignment.h:146-193), applies insert_new_path_pointer's `i>0 || j>0` rule
// (viterbi_alignment.h:196-200), marks the child edges the path used, and numbers the
// columns the way create_ancestral_sequence consumes them (basic_alignment.cpp:73-171).
int replay(const HostJob &hj, const int *endcell, double endscore, const int *trace, pagan_result *out) {
    const pagan_graph *L = hj.L, *R = hj.R;
    const int Lx = hj.Lx, Ly = hj.Ly;
    std::memset(out, 0, sizeof(*out));
    out->cells = hj.dx.cells;
    out->score = endscore;
    // nothing the device wrote is used as an index before it has been checked against the graphs
    if (endcell[0] != 0 && endcell[0] != 1) {
        if (std::getenv("PAGAN_DP_VERBOSE")) std::fprintf(stderr, "pagan_dp: device status %d\n", endcell[0]);
        return PAGAN_E_INTERNAL;
    }
    const int degL = L->bwd_off[Lx + 1] - L->bwd_off[Lx], degR = R->bwd_off[Ly + 1] - R->bwd_off[Ly];
    if (endcell[4] >= degL || endcell[5] >= degR) return PAGAN_E_INTERNAL;
    out->end_matrix = endcell[1]; out->end_x = endcell[2]; out->end_y = endcell[3];
    out->end_x_edge = endcell[4] >= 0 ? L->bwd_eid[L->bwd_off[Lx] + endcell[4]] : -1;
    out->end_y_edge = endcell[5] >= 0 ? R->bwd_eid[R->bwd_off[Ly] + endcell[5]] : -1;
    if (endcell[0] == 1) { out->status = PAGAN_DP_UNREACHABLE; return PAGAN_OK; }
    const int n = endcell[6];
    if (out->end_matrix < PAGAN_X_MAT || out->end_matrix > PAGAN_M_MAT || out->end_x < 0 || out->end_x >= Lx ||
        out->end_y < 0 || out->end_y >= Ly || n < 0 || n > Lx + Ly) return PAGAN_E_INTERNAL;

    std::vector<char> lused(L->n_edges, 0), rused(R->n_edges, 0);
    struct Step { int8_t matrix; int8_t real; };
    std::vector<Step> stack;
    stack.reserve((size_t)Lx + Ly);
    auto find_edge = [](const pagan_graph *g, int start, int site) {
        for (int k = g->bwd_off[site]; k < g->bwd_off[site + 1]; ++k)
            if (g->bwd_src[k] == start) return g->bwd_eid[k];
        return -1;
    };
    if (out->end_x_edge >= 0) lused[out->end_x_edge] = 1;              // VA:1054-1057
    if (out->end_y_edge >= 0) rused[out->end_y_edge] = 1;
    int i = Lx - 1, j = Ly - 1;
    int x_ind = endcell[2], y_ind = endcell[3];
    bool first_x = true, first_y = true;
    auto skips = [&](int xi, int yi) {
        while (xi < i) { stack.push_back({PAGAN_X_MAT, 0}); --i; }
        while (yi < j) { stack.push_back({PAGAN_Y_MAT, 0}); --j; }
    };
    auto push = [&](int matrix) { if (i > 0 || j > 0) stack.push_back({(int8_t)matrix, 1}); };
    skips(x_ind, y_ind);
    push(endcell[1]);
    for (int t = 0; t < n; ++t) {
        const int ci = trace[3 * t], cj = trace[3 * t + 1];
        const unsigned w = (unsigned)trace[3 * t + 2];
        const int vit = (int)(w & 3u), k1 = (int)((w >> 4) & 16383u), k2 = (int)(w >> 18);
        if (ci != i || cj != j || i < 0 || j < 0) return PAGAN_E_INTERNAL;
        if ((vit != PAGAN_Y_MAT && (i < 1 || k1 >= L->bwd_off[i + 1] - L->bwd_off[i])) ||
            (vit != PAGAN_X_MAT && (j < 1 || k2 >= R->bwd_off[j + 1] - R->bwd_off[j]))) return PAGAN_E_INTERNAL;
        // the cell's `from` label is the matrix of the next visited cell; for the last one
        // it is never pushed (i<1 && j<1 after it), so any value does
        const int from = (t + 1 < n) ? (int)((unsigned)trace[3 * (t + 1) + 2] & 3u) : PAGAN_M_MAT;
        if (vit == PAGAN_M_MAT) {
            if (first_x) { int e = find_edge(L, x_ind, Lx); if (e >= 0) lused[e] = 1; first_x = false; }
            if (first_y) { int e = find_edge(R, y_ind, Ly); if (e >= 0) rused[e] = 1; first_y = false; }
            const int el = L->bwd_off[i] + k1, er = R->bwd_off[j] + k2;
            x_ind = L->bwd_src[el]; y_ind = R->bwd_src[er];
            lused[L->bwd_eid[el]] = 1; rused[R->bwd_eid[er]] = 1;
            --i; --j;
        } else if (vit == PAGAN_X_MAT) {
            if (first_x) { int e = find_edge(L, x_ind, Lx); if (e >= 0) lused[e] = 1; first_x = false; }
            const int el = L->bwd_off[i] + k1;
            x_ind = L->bwd_src[el]; y_ind = j;
            lused[L->bwd_eid[el]] = 1;
            --i;
        } else if (vit == PAGAN_Y_MAT) {
            if (first_y) { int e = find_edge(R, y_ind, Ly); if (e >= 0) rused[e] = 1; first_y = false; }
            const int er = R->bwd_off[j] + k2;
            y_ind = R->bwd_src[er]; x_ind = i;
            rused[R->bwd_eid[er]] = 1;
            --j;
        } else {
            return PAGAN_E_INTERNAL;
        }
        skips(x_ind, y_ind);
        push(from);
    }
    if (!(i < 1 && j < 1)) return PAGAN_E_INTERNAL;

    out->n_cols = (int32_t)stack.size();
    out->cols = (pagan_col *)std::malloc(sizeof(pagan_col) * (stack.size() + 1));
    if (!out->cols) return PAGAN_E_NOMEM;
    int l_pos = 1, r_pos = 1;
    for (size_t k = 0; k < stack.size(); ++k) {
        const Step &s = stack[stack.size() - 1 - k];
        pagan_col c;
        if (s.matrix == PAGAN_X_MAT) { c.left = l_pos++; c.right = -1; c.path_state = s.real ? PAGAN_XGAPPED : PAGAN_XSKIPPED; }
        else if (s.matrix == PAGAN_Y_MAT) { c.left = -1; c.right = r_pos++; c.path_state = s.real ? PAGAN_YGAPPED : PAGAN_YSKIPPED; }
        else { c.left = l_pos++; c.right = r_pos++; c.path_state = PAGAN_MATCHED; }
        out->cols[k] = c;
    }
    if (l_pos != Lx || r_pos != Ly) { std::free(out->cols); out->cols = nullptr; return PAGAN_E_INTERNAL; }
    auto collect = [](const std::vector<char> &u, int32_t *cnt, int32_t **arr) {
        int c = 0;
        for (char x : u) c += x;
        *arr = (int32_t *)std::malloc(sizeof(int32_t) * (c + 1));
        int k = 0;
        for (size_t e = 0; e < u.size(); ++e) if (u[e]) (*arr)[k++] = (int32_t)e;
        *cnt = c;
    };
    collect(lused, &out->n_left_used, &out->left_used);
    collect(rused, &out->n_right_used, &out->right_used);
    out->status = PAGAN_DP_REACHED;
    return PAGAN_OK;
}

} // namespace

// The traceback's host half for callers outside this file (dp_fb.hip: a sampled path has the same shape as a
// Viterbi path): endcell / trace in the device's format (dp_device.h).
int pagan_internal_replay(const pagan_graph *L, const pagan_graph *R, int64_t cells, const int *endcell, double endscore,
                          const int *trace, pagan_result *out) {
    HostJob hj;
    hj.L = L; hj.R = R; hj.Lx = L->n_sites - 1; hj.Ly = R->n_sites - 1;
    hj.dx.cells = cells;
    return replay(hj, endcell, endscore, trace, out);
}

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

// Dead sites out of one job (see CompactJob): fills `cj` and points `eff` at the compacted graphs / band when the job
// qualifies (5 % dead sites or more, nothing validate_job would refuse).
static void compact_job(const pagan_job &jb, bool allow, CompactJob *cjp, pagan_job *eff) {
    CompactJob &cj = *cjp;
    if (!allow || !jb.left || !jb.right || !jb.model) return;
    if (check_graph(jb.left) != PAGAN_OK || check_graph(jb.right) != PAGAN_OK) return;     // validate_job reports it
    const int nl = jb.left->n_sites, nr = jb.right->n_sites;
    int dl = 0, dr = 0;
    for (int s_ = 1; s_ + 2 < nl; ++s_) dl += jb.left->bwd_off[s_ + 1] == jb.left->bwd_off[s_];
    for (int s_ = 1; s_ + 2 < nr; ++s_) dr += jb.right->bwd_off[s_ + 1] == jb.right->bwd_off[s_];
    if (20 * (dl + dr) < nl + nr) return;                      // under 5 %: not worth the copies
    // (what validate_job would refuse on the caller's graphs must not slip through on the smaller ones)
    for (int s_ = 1; s_ + 1 < nl; ++s_) if (jb.left->state[s_] < 0 || jb.left->state[s_] >= jb.model->n_states) return;
    for (int s_ = 1; s_ + 1 < nr; ++s_) if (jb.right->state[s_] < 0 || jb.right->state[s_] >= jb.model->n_states) return;
    RowBand rb0;
    if (rb0.build(nl - 1, nr - 1, jb.band) != PAGAN_OK) return;
    cj.cells0 = rb0.cells();
    cj.L0 = jb.left; cj.R0 = jb.right;
    cj.l.build(jb.left); cj.r.build(jb.right);
    eff->left = &cj.l.g; eff->right = &cj.r.g;
    if (jb.band) {
        compact_band(rb0, cj.l, cj.r, nr, &cj.up, &cj.lo);
        const int rows = (int)cj.up.size();
        cj.band.n = rows; cj.band.upper = cj.up.data(); cj.band.lower = cj.lo.data();
        eff->band = &cj.band;
    }
    cj.on = true;
}

// Host-only: which fill kernel pagan_batch_create would give this job -- 0 pg_fill_pipe (model table in LDS), 1 pg_fill_pipe
// (large table), 2 pg_fill_tiles_flow, 3 pg_fill_wavefront -- after taking its dead sites out as the batch does; negative: the
// error validate_job reports.  n_out[0] = 1 when the job is aligned on compacted graphs, n_out[1] = widest diagonal.
int pagan_dp_debug_route(const pagan_graph *left, const pagan_graph *right, const pagan_model *model, const pagan_band *band,
                         int32_t *n_out) {
    pagan_job jb;
    std::memset(&jb, 0, sizeof(jb));
    jb.left = left; jb.right = right; jb.model = model; jb.band = band;
    pagan_job eff = jb;
    CompactJob cj;
    const char *ce = std::getenv("PAGAN_DP_COMPACT");
    compact_job(jb, !(ce && std::strcmp(ce, "0") == 0), &cj, &eff);
    HostJob hj;
    RowBand rb;
    bool use_pipe = true;
    if (const char *f = std::getenv("PAGAN_DP_FILL")) use_pipe = std::strcmp(f, "ring") != 0;
    const int rc = validate_job(eff, &hj, &rb, use_pipe);
    if (rc != PAGAN_OK) return rc;
    if (n_out) { n_out[0] = cj.on ? 1 : 0; n_out[1] = hj.dx.max_width; }
    const char *wide_env = std::getenv("PAGAN_DP_WIDE");
    const bool use_tiles = !std::getenv("PAGAN_DP_FORCE_GLOBAL_WAVEFRONT") && !(wide_env && std::strcmp(wide_env, "wavefront") == 0);
    if (hj.ring_ok && !std::getenv("PAGAN_DP_FORCE_GLOBAL_WAVEFRONT")) return eff.model->n_states <= 16 ? 0 : 1;
    if (use_tiles && !hj.strips.empty()) return 4;
    if (use_tiles && !hj.tiles.empty()) return 2;
    return 3;
}

// Host-only: the per-diagonal classes and the wave schedule pg_fill_pipe would be given for this job
// (what validate_job computes); lets the planner be tested without a device.
int pagan_dp_debug_plan(const pagan_graph *left, const pagan_graph *right, const pagan_band *band, uint8_t *cls_out,
                        int32_t n_cls, int32_t *sched_out, int32_t sched_cap, int32_t *sched_len, int32_t *lead_req_out) {
    if (!left || !right || !cls_out || !sched_out || !sched_len) return PAGAN_E_ARG;
    int rc;
    if ((rc = check_graph(left)) != PAGAN_OK) return rc;
    if ((rc = check_graph(right)) != PAGAN_OK) return rc;
    const int Lx = left->n_sites - 1, Ly = right->n_sites - 1;
    if (n_cls != Lx + Ly - 1) return PAGAN_E_ARG;
    static const bool prof = std::getenv("PAGAN_DP_PLAN_PROFILE") != nullptr;
    auto t_last = std::chrono::steady_clock::now();
    auto lap = [&](const char *what) {
        if (!prof) return;
        const auto t = std::chrono::steady_clock::now();
        std::fprintf(stderr, "pagan_dp: plan %s %.2f ms\n", what, std::chrono::duration<double, std::milli>(t - t_last).count());
        t_last = t;
    };
    lap("checks");
    RowBand rb;
    if ((rc = rb.build(Lx, Ly, band)) != PAGAN_OK) return rc;
    lap("row band");
    DiagIndex dx;
    dx.build(Lx, Ly, rb);
    lap("diagonal index");
    std::vector<uint8_t> cls;
    std::vector<int> sched, lead_req;
    int threads = 1;                                            // PAGAN_DP_PLAN_THREADS: the plan over several threads (tests compare with one)
    if (const char *e = std::getenv("PAGAN_DP_PLAN_THREADS")) threads = std::max(1, std::atoi(e));
    classify_diagonals(left, right, Lx, Ly, rb, dx, true, &cls, &lead_req, nullptr, threads);      // the plan of a job whose model table fits LDS
    lap("classify_diagonals");
    schedule_waves(dx, cls, &sched, threads);
    lap("schedule_waves");
    std::memcpy(cls_out, cls.data(), cls.size());
    if (lead_req_out) std::memcpy(lead_req_out, lead_req.data(), sizeof(int) * lead_req.size());
    *sched_len = (int32_t)sched.size();
    if ((int)sched.size() > sched_cap) return PAGAN_E_ARG;
    std::memcpy(sched_out, sched.data(), sizeof(int) * sched.size());
    return PAGAN_OK;
}

int pagan_dp_debug_far(const pagan_graph *left, const pagan_graph *right, const pagan_band *band,
                       uint8_t *hfL, uint8_t *hfR, uint8_t *hbit, uint8_t *cls_out) {
    if (!left || !right || !hfL || !hfR || !hbit || !cls_out) return PAGAN_E_ARG;
    int rc;
    if ((rc = check_graph(left)) != PAGAN_OK) return rc;
    if ((rc = check_graph(right)) != PAGAN_OK) return rc;
    const int Lx = left->n_sites - 1, Ly = right->n_sites - 1;
    RowBand rb;
    if ((rc = rb.build(Lx, Ly, band)) != PAGAN_OK) return rc;
    DiagIndex dx;
    dx.build(Lx, Ly, rb);
    std::vector<uint8_t> cls;
    std::vector<int> lead_req;
    FarPlan fp;
    classify_diagonals(left, right, Lx, Ly, rb, dx, true, &cls, &lead_req, nullptr, 1, &fp);
    std::memcpy(hfL, fp.hfL.data(), fp.hfL.size()); std::memcpy(hfR, fp.hfR.data(), fp.hfR.size());
    for (size_t d = 0; d < fp.hbit.size(); ++d) hbit[d] = (uint8_t)(fp.hbit[d] | (fp.tbit.size() > d && fp.tbit[d] ? 2 : 0));     // bit 1: the third pass
    std::memcpy(cls_out, cls.data(), cls.size());
    return fp.n_served;
}

int pagan_dp_debug_strips(const pagan_graph *left, const pagan_graph *right, const pagan_band *band, int32_t max_sites,
                          int32_t *strips, int32_t cap, int64_t *desc_off, int64_t *desc, int64_t desc_cap) {
    if (!left || !right || !strips || !desc_off || !desc || cap < 0 || desc_cap < 0) return PAGAN_E_ARG;
    int rc;
    if ((rc = check_graph(left)) != PAGAN_OK) return rc;
    if ((rc = check_graph(right)) != PAGAN_OK) return rc;
    const int Lx = left->n_sites - 1, Ly = right->n_sites - 1;
    RowBand rb;
    if ((rc = rb.build(Lx, Ly, band)) != PAGAN_OK) return rc;
    DiagIndex dx;
    dx.build(Lx, Ly, rb);
    std::vector<StripPlan> plan;
    int seen = 0;
    if (!plan_strips(left, right, Lx, Ly, rb, dx, &plan, max_sites > 0 ? max_sites : (1 << 30), &seen, false)) return 0;
    if ((int)plan.size() > cap) return PAGAN_E_ARG;
    int64_t at = 0;
    for (size_t k = 0; k < plan.size(); ++k) {
        const StripPlan &sp = plan[k];
        int32_t *o = strips + 6 * k;
        o[0] = sp.r0; o[1] = sp.r1; o[2] = sp.d0; o[3] = sp.d1; o[4] = sp.feed_wave; o[5] = sp.col_first;
        desc_off[k] = at;
        const int m = sp.d1 - sp.d0;
        if (at + m > desc_cap) return PAGAN_E_ARG;
        for (int t = 0; t < m; ++t) {
            const int *pk = sp.psc.data() + 8 * (size_t)t;
            const long long boff = ((long long)pk[3] << 32) | (unsigned)pk[2];
            int64_t *e = desc + 4 * (at + t);
            e[0] = pk[0]; e[1] = pk[1]; e[2] = boff / 24; e[3] = pk[4] & 7;
        }
        at += m;
    }
    desc_off[plan.size()] = at;
    return (int)plan.size();
}

int pagan_dp_debug_tiles(const pagan_graph *left, const pagan_graph *right, const pagan_band *band, int32_t *tiles,
                         int32_t cap, int32_t *tile_side) {
    if (!left || !right || !tiles || cap < 0) return PAGAN_E_ARG;
    int rc;
    if ((rc = check_graph(left)) != PAGAN_OK) return rc;
    if ((rc = check_graph(right)) != PAGAN_OK) return rc;
    const int Lx = left->n_sites - 1, Ly = right->n_sites - 1;
    RowBand rb;
    if ((rc = rb.build(Lx, Ly, band)) != PAGAN_OK) return rc;
    if (tile_side) *tile_side = PG_TILE;
    if (!edges_fit_tiles(left, Lx) || !edges_fit_tiles(right, Ly)) return 0;
    std::vector<int> list;
    list_tiles(Lx, rb, &list);
    const int n = (int)(list.size() / 2);
    std::memcpy(tiles, list.data(), sizeof(int) * 2 * (size_t)std::min(n, (int)cap));
    return n;
}

int pagan_dp_debug_tiles_staircase(const int32_t *tiles, int32_t n) {
    if (!tiles || n < 0) return PAGAN_E_ARG;
    return tiles_staircase(std::vector<int>(tiles, tiles + 2 * (size_t)n)) ? 1 : 0;
}

int pagan_dp_debug_compact(const pagan_graph *left, const pagan_graph *right, const pagan_band *band, int32_t *keep_left,
                           int32_t *keep_right, int32_t *slot_left, int32_t *slot_right, int32_t *upper, int32_t *lower,
                           int32_t *n_out /* [4]: kept left sites, kept right sites, kept left edges, kept right edges */) {
    if (!left || !right || !n_out) return PAGAN_E_ARG;
    int rc;
    if ((rc = check_graph(left)) != PAGAN_OK) return rc;
    if ((rc = check_graph(right)) != PAGAN_OK) return rc;
    CompactSide l, r;
    l.build(left); r.build(right);
    n_out[0] = (int32_t)l.keep.size(); n_out[1] = (int32_t)r.keep.size();
    n_out[2] = (int32_t)l.slot.size(); n_out[3] = (int32_t)r.slot.size();
    if (keep_left) std::copy(l.keep.begin(), l.keep.end(), keep_left);
    if (keep_right) std::copy(r.keep.begin(), r.keep.end(), keep_right);
    if (slot_left) std::copy(l.slot.begin(), l.slot.end(), slot_left);
    if (slot_right) std::copy(r.slot.begin(), r.slot.end(), slot_right);
    if (upper && lower) {
        RowBand rb0;
        if ((rc = rb0.build(left->n_sites - 1, right->n_sites - 1, band)) != PAGAN_OK) return rc;
        std::vector<int> up, lo;
        compact_band(rb0, l, r, right->n_sites, &up, &lo);
        std::copy(up.begin(), up.end(), upper);
        std::copy(lo.begin(), lo.end(), lower);
    }
    return PAGAN_OK;
}

int64_t pagan_dp_count_cells(int32_t left_sites, int32_t right_sites, const pagan_band *band) {
    if (left_sites < 2 || right_sites < 2) return PAGAN_E_ARG;
    RowBand rb;
    int rc = rb.build(left_sites - 1, right_sites - 1, band);
    if (rc != PAGAN_OK) return rc;
    return rb.cells();
}

// Device bytes for one alignment (an upper bound of what carve_job / carve_outputs lay out): 36 B per in-band
// cell (3 x (f64 score + u32 back-pointer)) + at most 1.5 B per cell of traceback tables (32 B per state of the two
// boundary diagonals in every PG_SEG = 256: 0.75 B) + per diagonal 64 B of band index, descriptors and plan + per site 12 B of
// trace buffer and ~20 B of graph arrays (one to two bwd edges per site), all 256-byte aligned.
int64_t pagan_dp_predict_bytes(int32_t left_sites, int32_t right_sites, const pagan_band *band) {
    int64_t cells = pagan_dp_count_cells(left_sites, right_sites, band);
    if (cells < 0) return cells;
    const int64_t nd = (int64_t)left_sites + right_sites - 3, sites = (int64_t)left_sites + right_sites;
    return cells * 38 + nd * 64 + sites * 40 + 128 * 1024;
}

int pagan_batch_create(int32_t n, const pagan_job *jobs, const pagan_opts *opts, pagan_batch **out) {
    if (n <= 0 || !jobs || !out) return PAGAN_E_ARG;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return PAGAN_E_NODEVICE;
    pagan_batch *b = new (std::nothrow) pagan_batch();
    if (!b) return PAGAN_E_NOMEM;
    struct Guard { pagan_batch *b; ~Guard() { if (b) pagan_batch_destroy(b); } } guard{b};
    b->n = n;
    b->flags = opts ? opts->flags : 0;
    if (const char *e = std::getenv("PAGAN_DP_STRIP_SPREAD")) b->strips_spread = std::atoi(e) != 0;
    if (opts && opts->device >= 0) HIP_TRY(hipSetDevice(opts->device));
    HIP_TRY(hipGetDevice(&b->device));
    b->jobs.resize(n);
    b->dj.resize(n);
    int max_w = 0;
    const bool force_v1 = std::getenv("PAGAN_DP_FORCE_GLOBAL_WAVEFRONT") != nullptr;   // A/B switch for profiling
    // A/B switch: PAGAN_DP_FILL=ring runs the barrier-per-diagonal LDS kernel instead of the register wavefront
    if (const char *f = std::getenv("PAGAN_DP_FILL")) b->use_pipe = std::strcmp(f, "ring") != 0;
    if (const char *f = std::getenv("PAGAN_DP_BP")) b->bp_pass = std::strcmp(f, "verify") == 0 ? 2 : (std::strcmp(f, "fill") == 0 ? 0 : 1);
    // ("fill" = the fill kernel writes its own back-pointers: true of the ring kernel only -- pg_fill_pipe's loop stores scores
    //  and nothing else, so with it the pass always runs)
    if (b->use_pipe && b->bp_pass == 0) b->bp_pass = 1;
    if (const char *f = std::getenv("PAGAN_DP_DEBUG_FLAGS")) b->flags |= (uint32_t)std::strtoul(f, nullptr, 0) & 0xff00u;
    // A/B switch: PAGAN_DP_WIDE=wavefront sends the wide jobs to the one-workgroup HBM wavefront instead of the tiles
    const char *wide_env = std::getenv("PAGAN_DP_WIDE");
    const bool use_tiles = !force_v1 && !(wide_env && std::strcmp(wide_env, "wavefront") == 0);
    std::vector<int> which_ring, which_ring_big, which_wide, which_tiled, which_striped;
    std::vector<int> job_rc(n, PAGAN_OK);
    const bool verbose = std::getenv("PAGAN_DP_VERBOSE") != nullptr;
    auto now = [] { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    const double tc0 = now();
    // dead sites out (see CompactJob): the rest of this function works on the effective jobs
    std::vector<pagan_job> eff(jobs, jobs + n);
    b->compact.resize(n);
    {
        const char *ce = std::getenv("PAGAN_DP_COMPACT");
        const bool allow = !(ce && std::strcmp(ce, "0") == 0);
        parallel_jobs(n, [&](int k) { compact_job(jobs[k], allow, &b->compact[k], &eff[k]); });
    }
    {
        // a level of few alignments: the threads the jobs leave idle go into each job's own plan
        const int hw = (int)std::thread::hardware_concurrency();
        const int inner = std::max(1, std::min(8, (hw > 0 ? std::min(hw, 16) : 1) / std::max(n, 1)));
        parallel_jobs(n, [&](int k) {
            RowBand rb;
            job_rc[k] = validate_job(eff[k], &b->jobs[k], &rb, b->use_pipe, inner);
        });
    }
    for (int k = 0; k < n; ++k) {
        const int rc = job_rc[k];
        if (rc != PAGAN_OK) return rc;
        b->cells += b->compact[k].on ? b->compact[k].cells0 : b->jobs[k].dx.cells;       // the caller's cells
        if (b->jobs[k].n_bound > b->max_bound) b->max_bound = b->jobs[k].n_bound;
        b->max_path = std::max(b->max_path, b->jobs[k].Lx + b->jobs[k].Ly);
        if (b->jobs[k].n_bound > 0 && b->jobs[k].tb[b->jobs[k].n_bound + 1] > b->max_entries) b->max_entries = b->jobs[k].tb[b->jobs[k].n_bound + 1];
        if (b->jobs[k].ring_ok && !force_v1) {
            (eff[k].model->n_states <= 16 ? which_ring : which_ring_big).push_back(k);
            continue;
        }
        if (use_tiles && !b->jobs[k].ring_ok && !b->jobs[k].strips.empty()) { which_striped.push_back(k); continue; }
        if (use_tiles && !b->jobs[k].ring_ok && !b->jobs[k].tiles.empty()) { which_tiled.push_back(k); continue; }
        which_wide.push_back(k);
        if (b->jobs[k].dx.max_width > max_w) max_w = b->jobs[k].dx.max_width;
    }
    // tile launches: launch t takes the tiles with row + column = t of every tiled job
    std::vector<int> tile_list;
    if (!which_tiled.empty()) {
        int T = 0;
        for (int k : which_tiled) {
            const std::vector<int> &tl = b->jobs[k].tiles;
            for (size_t q = 0; q < tl.size(); q += 2) T = std::max(T, tl[q] + tl[q + 1] + 1);
        }
        b->tile_off.assign(T + 1, 0);
        for (int k : which_tiled) {
            const std::vector<int> &tl = b->jobs[k].tiles;
            for (size_t q = 0; q < tl.size(); q += 2) ++b->tile_off[tl[q] + tl[q + 1] + 1];
        }
        for (int t = 0; t < T; ++t) b->tile_off[t + 1] += b->tile_off[t];
        const size_t N = (size_t)b->tile_off[T];
        tile_list.assign(4 * N + 4 + 2 * N + (size_t)T + 1, 0);
        std::vector<int> cur(b->tile_off.begin(), b->tile_off.end() - 1);
        std::unordered_map<uint64_t, int> where;               // (job, tile row, tile column) -> position in the list
        where.reserve(2 * N);
        auto key = [](int k, int a, int bb) { return ((uint64_t)(uint32_t)k << 40) | ((uint64_t)(uint32_t)a << 20) | (uint64_t)(uint32_t)bb; };
        for (int k : which_tiled) {
            const std::vector<int> &tl = b->jobs[k].tiles;
            for (size_t q = 0; q < tl.size(); q += 2) {
                const int pos = cur[tl[q] + tl[q + 1]]++;
                const size_t at = 4 * (size_t)pos;
                tile_list[at] = k; tile_list[at + 1] = tl[q]; tile_list[at + 2] = tl[q + 1];
                where[key(k, tl[q], tl[q + 1])] = pos;
            }
        }
        // pg_fill_tiles_flow: the tiles above and to the left (list positions, -1: not in the band), the diagonals' offsets
        for (size_t pos = 0; pos < N; ++pos) {
            const int k = tile_list[4 * pos], a = tile_list[4 * pos + 1], bb = tile_list[4 * pos + 2];
            auto up = a > 0 ? where.find(key(k, a - 1, bb)) : where.end();
            auto lf = bb > 0 ? where.find(key(k, a, bb - 1)) : where.end();
            auto dg = a > 0 && bb > 0 ? where.find(key(k, a - 1, bb - 1)) : where.end();
            tile_list[4 * pos + 3] = up == where.end() ? -1 : up->second;
            tile_list[4 * N + 4 + pos] = lf == where.end() ? -1 : lf->second;
            tile_list[4 * N + 4 + N + pos] = dg == where.end() ? -1 : dg->second;
        }
        for (int t = 0; t <= T; ++t) tile_list[4 * N + 4 + 2 * N + (size_t)t] = b->tile_off[t];
        // The neighbour flags alone order a tile behind everything it can read only if the job's tiles form a staircase
        // (dp_tiles.hip): every tile row a contiguous run of columns, first and last column never falling from one row to
        // the next, no empty row between two rows, consecutive rows touching.
        for (int k : which_tiled) {
            const bool stair = tiles_staircase(b->jobs[k].tiles);
            if (!stair) b->tiles_water = true;
        }
        if (const char *f = std::getenv("PAGAN_DP_TILES")) if (std::strcmp(f, "watermark") == 0) b->tiles_water = true;
        if (const char *f = std::getenv("PAGAN_DP_TILES")) if (std::strcmp(f, "nolag") == 0) b->tiles_nolag = true;
        b->flow_ints = 1 + (size_t)T + N + 1;                  // queue head, finished tiles per diagonal, progress per tile, give-up flag
        if (const char *f = std::getenv("PAGAN_DP_TILES")) b->tiles_flow = std::strcmp(f, "launches") != 0;   // A/B switch
    }
    b->n_ring_small = (int)which_ring.size();
    which_ring.insert(which_ring.end(), which_ring_big.begin(), which_ring_big.end());
    b->n_ring = (int)which_ring.size(); b->n_wide = (int)which_wide.size();
    which_ring.insert(which_ring.end(), which_wide.begin(), which_wide.end());
    b->n_striped = (int)which_striped.size();
    b->n_tiled = (int)which_striped.size() + (int)which_tiled.size();
    which_ring.insert(which_ring.end(), which_striped.begin(), which_striped.end());  // (striped and tiled jobs: one back-pointer pass behind both fills)
    which_ring.insert(which_ring.end(), which_tiled.begin(), which_tiled.end());     // (the tiled fill reaches its jobs through the tile list; pg_backptr through this)
    // Row strips: every strip a device job of its own behind the batch's n; the strips of a job at workgroup indices of one
    // residue mod 8 (one XCD: a strip reads what the strip above stored from that XCD's L2), in order
    struct StripDev { int job, q; int *psc, *sched, *follow; };
    std::vector<StripDev> sdev;
    std::vector<int> swhich;
    {
        // a job to the XCD with the least work so far (largest jobs first); inside an XCD's list the strips of its jobs by
        // first diagonal: workgroups are dispatched in index order and a strip holds its compute unit while it waits for the
        // strip above, so what is resident should be what can run -- the fronts of all the XCD's jobs, not one job's whole
        // chain.  (A job's strips stay in order: their first diagonals grow.)  A strip's device job is found through `where`.
        // device jobs of the strips: job-major (a strip finds the strip above in the entry before its own)
        std::unordered_map<long long, int> where;
        for (int k : which_striped)
            for (size_t q = 0; q < b->jobs[k].strips.size(); ++q) {
                where[((long long)k << 20) | (long long)q] = n + (int)sdev.size();
                sdev.push_back({k, (int)q, nullptr, nullptr, nullptr});
            }
        // two dispatches: the jobs whose model table fits LDS (pg_fill_pipe<true, true>), then the others (<false, true>)
        for (int big = 0; big < 2; ++big) {
            std::vector<int> by_size;
            for (int k : which_striped) if ((eff[k].model->n_states * eff[k].model->n_states > 256) == (big == 1)) by_size.push_back(k);
            std::stable_sort(by_size.begin(), by_size.end(), [&](int a, int c) { return b->jobs[a].dx.cells > b->jobs[c].dx.cells; });
            long long lane_cells[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            std::vector<std::vector<std::pair<int, int>>> lane_strips(8);          // (job, strip)
            for (int k : by_size) {
                int lane = 0;
                for (int x = 1; x < 8; ++x) if (lane_cells[x] < lane_cells[lane]) lane = x;
                lane_cells[lane] += b->jobs[k].dx.cells;
                for (size_t q = 0; q < b->jobs[k].strips.size(); ++q) lane_strips[lane].push_back({k, (int)q});
            }
            const size_t first = swhich.size();                          // (a multiple of 8)
            if (b->strips_spread) {
                // PAGAN_DP_STRIP_SPREAD (the default, round 5): a job's strips on ANY XCD -- they store their scores through to
                // memory and read the strip above's with sc1 loads (dp_pipe.hip, store_scores / strip_feeder), so a single wide job
                // (the root of a tree) has the whole chip, not one XCD's 32 units.  All strips of the launch in the order of their
                // first diagonals: the order they can start in (a job's own strips stay in order: their first diagonals grow).
                std::vector<std::pair<int, int>> all;
                for (int lane = 0; lane < 8; ++lane) all.insert(all.end(), lane_strips[lane].begin(), lane_strips[lane].end());
                std::stable_sort(all.begin(), all.end(), [&](const std::pair<int, int> &a, const std::pair<int, int> &c) {
                    const int da = b->jobs[a.first].strips[a.second].d0, dc = b->jobs[c.first].strips[c.second].d0;
                    return da != dc ? da < dc : (a.first != c.first ? a.first < c.first : a.second < c.second); });
                for (const auto &js : all) swhich.push_back(where[((long long)js.first << 20) | (long long)js.second]);
                while (swhich.size() % 8) swhich.push_back(-1);
            } else
            for (int lane = 0; lane < 8; ++lane) {
                auto &ls = lane_strips[lane];
                std::stable_sort(ls.begin(), ls.end(), [&](const std::pair<int, int> &a, const std::pair<int, int> &c) {
                    return b->jobs[a.first].strips[a.second].d0 < b->jobs[c.first].strips[c.second].d0; });
                for (size_t pos = 0; pos < ls.size(); ++pos) {
                    const size_t at = first + 8 * pos + lane;
                    if (swhich.size() <= at) swhich.resize(first + ((at - first) / 8 + 1) * 8, -1);
                    swhich[at] = where[((long long)ls[pos].first << 20) | (long long)ls[pos].second];
                }
            }
            (big ? b->strip_grid_big : b->strip_grid) = (int)(swhich.size() - first);
        }
        b->dj.resize((size_t)n + sdev.size());
    }
    which_ring.resize(n, 0);
    b->block = max_w <= 64 ? 64 : (max_w <= 512 ? 256 : 1024);

    const double tc1 = now();
    // pass 1: sizes.  Inputs first (one contiguous upload), outputs after.
    Carver sizer;
    if (const char *cm = std::getenv("PAGAN_DP_CANARY")) if (std::strcmp(cm, "0") != 0) {
        sizer.guards = &b->guards;
        if (cm[0] == '0' && cm[1] == 'x') b->canary_word = (unsigned)std::strtoul(cm, nullptr, 16);
    }
    PgDevJob *jobs_off = sizer.take<PgDevJob>((size_t)n + sdev.size());
    int *which_off = sizer.take<int>(n);
    int *swhich_off = sizer.take<int>(swhich.size());
    for (StripDev &sd : sdev) {
        const StripPlan &sp = b->jobs[sd.job].strips[sd.q];
        sd.psc = sizer.take<int>(sp.psc.size()); sd.sched = sizer.take<int>(sp.sched.size());
    }
    int *tiles_off = sizer.take<int>(tile_list.size());
    int *flow_off = sizer.take<int>(b->flow_ints);
    for (int k = 0; k < n; ++k) carve_job(sizer, eff[k], b->jobs[k], &b->dj[k]);
    const size_t in_bytes = sizer.cur;
    b->out_begin = in_bytes;
    for (int k = 0; k < n; ++k) carve_outputs(sizer, b->jobs[k], &b->dj[k]);
    carve_ends(sizer, n, b->dj.data());
    carve_follow(sizer, n, b->jobs, b->dj.data(), &b->follow_begin, &b->follow_bytes);
    b->sfollow_begin = sizer.cur;
    for (StripDev &sd : sdev) sd.follow = sizer.take<int>(4);
    b->sfollow_bytes = sizer.cur - b->sfollow_begin;
    b->arena.size = sizer.cur;
    b->arena.dev = arena_pool.take(b->device, b->arena.size, &b->arena.cap);
    if (!b->arena.dev) {
        b->arena.cap = b->arena.size;
        if (hipMalloc((void **)&b->arena.dev, b->arena.size) != hipSuccess) {
            (void)hipGetLastError();
            b->arena.dev = nullptr;
            arena_pool.clear(b->device);                 // the idle arenas may be what is in the way -- and the other pools' (parent
            pagan::parent_release_cache();               // builder slabs, forward/backward arenas: round 4 advisor)
            pagan_fb_internal_release_cache();
            HIP_TRY(hipMalloc((void **)&b->arena.dev, b->arena.size));
        }
    }
    if (!b->guards.empty()) {
        // (the follow words are zeroed in one sweep per run, guards and all: those regions go unguarded)
        auto zeroed = [&](size_t o) { return (o >= b->follow_begin && o < b->follow_begin + b->follow_bytes) || (o >= b->sfollow_begin && o < b->sfollow_begin + b->sfollow_bytes); };
        b->guards.erase(std::remove_if(b->guards.begin(), b->guards.end(), zeroed), b->guards.end());
        HIP_TRY(hipMalloc((void **)&b->d_guards, b->guards.size() * sizeof(size_t)));
        HIP_TRY(hipMalloc((void **)&b->d_canary, 2 * sizeof(int)));
        HIP_TRY(hipMemcpy(b->d_guards, b->guards.data(), b->guards.size() * sizeof(size_t), hipMemcpyHostToDevice));
    }
    const double tc2 = now();

    // pass 2: stage inputs (offsets from pass 1 index the staging buffer), then rebase.
    Stage stage(in_bytes);
    if (!stage.data()) return PAGAN_E_NOMEM;
    parallel_jobs(n, [&](int k) {
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
            int *packed = reinterpret_cast<int *>(stage.data() + reinterpret_cast<size_t>(d.psc));
            std::memset(packed + 8 * hj.dx.imin.size(), 0, 8 * sizeof(int));                             // the entry of padding
            unsigned mask = 0;             // bit a: diagonal t-a was computed by the lanes (class <= 3), a = 1 .. REACH-1
            // hop[t]: how many of its own diagonals (t + PNA, t + 2 PNA, ...) an assist wave may skip after t before the
            // next one with work for it (a multi-edge cell, or -- model table too large for LDS -- any interior diagonal);
            // 12 bits, saturating: it looks again after a saturated hop
            const size_t ndg = hj.dx.imin.size();
            const bool big_table = d.S * d.S > 256;
            // wide runs (consecutive class 4 diagonals): does any diagonal of the run exceed PG_PIPE_WINDOW_A cells?  (bit 4 of a class
            // 4 diagonal's word: wide_run takes the wide-ring geometry with more positions and fewer rows then.)  Bit 19: the run has
            // at least PG_PIPE_ASSIST diagonals (small tables) -- every assist wave meets one of them, and the run is wide_run7's:
            // the assist waves take rows of their own.  PAGAN_DP_WIDE7=0: every run stays with the four compute waves (A/B switch)
            const bool wide7_on = !(std::getenv("PAGAN_DP_WIDE7") && std::strcmp(std::getenv("PAGAN_DP_WIDE7"), "0") == 0);
            std::vector<uint8_t> wide_b(ndg, 0), wide7(ndg, 0);
            for (size_t t = 0; t < ndg;) {
                if (hj.cls[t] != 4) { ++t; continue; }
                size_t e = t;
                int widest = 0;
                while (e < ndg && hj.cls[e] == 4) { widest = std::max(widest, hj.dx.imax[e] - hj.dx.imin[e] + 1); ++e; }
                if (widest > PG_PIPE_WINDOW_A) for (size_t q = t; q < e; ++q) wide_b[q] = 1;
                if (wide7_on && !big_table && e - t >= (size_t)PG_PIPE_ASSIST) for (size_t q = t; q < e; ++q) wide7[q] = 1;
                t = e;
            }
            // ... and the runs of class 5 diagonals (widest_run7: the same cells over 448 lanes)
            for (size_t t = 0; t < ndg && wide7_on && !big_table;) {
                if (hj.cls[t] != 5) { ++t; continue; }
                size_t e = t;
                while (e < ndg && hj.cls[e] == 5) ++e;
                if (e - t >= (size_t)PG_PIPE_ASSIST) for (size_t q = t; q < e; ++q) wide7[q] = 1;
                t = e;
            }
            std::vector<int> hop(ndg, 0);
            for (size_t t = ndg; t-- > 0;) {
                const size_t nx = t + PG_PIPE_ASSIST;
                if (nx >= ndg) { hop[t] = 4095; continue; }
                const bool work = hj.cls[nx] == 2 || (big_table && hj.cls[nx] <= 1) || wide7[nx];     // small tables: class 1 is the compute waves' own
                hop[t] = work ? 1 : std::min(4095, hop[nx] + 1);
            }
            for (size_t t = 0; t < hj.dx.imin.size(); ++t) {
                packed[8 * t] = hj.dx.imin[t]; packed[8 * t + 1] = hj.dx.imax[t];
                const long long boff = 24 * hj.dx.doff[t];
                packed[8 * t + 2] = (int)(boff & 0xffffffffLL); packed[8 * t + 3] = (int)(boff >> 32);
                // (a wide diagonal reuses the ring's memory: nothing older than it is resident afterwards)
                mask = (t >= 1 && hj.cls[t - 1] <= 3) ? (((mask << 1) | 2u) & (((1u << PG_PIPE_REACH) - 1u) & ~1u)) : 0u;
                // bit 4: large tables -- the next step is hot too; small tables -- a class 2 diagonal with every operand in the ring
                const unsigned pair = big_table ? (t + 1 < hj.cls.size() && hj.cls[t + 1] <= 2 ? 1u : 0u) : ((hj.ring2[t] || wide_b[t]) ? 1u : 0u);
                // bit 5 (bit 0 of the residency mask, which no age uses): a far history's writer or reader has a cell on the diagonal
                const unsigned hb = (!hj.hbit.empty() && hj.hbit[t]) ? 1u : 0u;
                // bit 19 (above the mask's REACH - 1 ages): a three-edge site of the lanes' third pass has a cell on the diagonal
                const unsigned tb = ((!hj.tbit.empty() && hj.tbit[t]) || wide7[t]) ? 1u : 0u;      // (class 4: a seven-wave wide run)
                static_assert(PG_PIPE_REACH <= 14, "descriptor word 4: ages 1 .. REACH - 1 in bits 6 .. 18, bit 19 for the third pass");
                packed[8 * t + 4] = (int)(hj.cls[t] | (pair << 4) | ((mask | hb) << 5) | (tb << 19) | ((unsigned)hop[t] << 20));
                packed[8 * t + 5] = (int)(hj.dx.doff[t] & 0xffffffffLL); packed[8 * t + 6] = (int)(hj.dx.doff[t] >> 32);
                packed[8 * t + 7] = hj.lead_req[t];
            }
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
    const double tc3 = now();
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
    std::memcpy(stage.data() + reinterpret_cast<size_t>(jobs_off), b->dj.data(), sizeof(PgDevJob) * b->dj.size());
    std::memcpy(stage.data() + reinterpret_cast<size_t>(which_off), which_ring.data(), sizeof(int) * n);
    if (!swhich.empty()) std::memcpy(stage.data() + reinterpret_cast<size_t>(swhich_off), swhich.data(), sizeof(int) * swhich.size());
    b->d_swhich = reinterpret_cast<int *>(base + reinterpret_cast<size_t>(swhich_off));
    b->d_jobs = reinterpret_cast<PgDevJob *>(base + reinterpret_cast<size_t>(jobs_off));
    b->d_which = reinterpret_cast<int *>(base + reinterpret_cast<size_t>(which_off));
    if (!tile_list.empty()) std::memcpy(stage.data() + reinterpret_cast<size_t>(tiles_off), tile_list.data(), sizeof(int) * tile_list.size());
    b->d_tiles = reinterpret_cast<int *>(base + reinterpret_cast<size_t>(tiles_off));
    b->d_flow = reinterpret_cast<int *>(base + reinterpret_cast<size_t>(flow_off));
    {
        // streams and events come from a per-device pool: a level of a tree walk is followed by the next, and creating and
        // destroying a dozen of them per batch cost milliseconds of the walk's wall-clock
        GpuObjs o;
        if (!gpu_pool.take(b->device, &o)) {
            HIP_TRY(hipStreamCreate(&o.stream));
            HIP_TRY(hipStreamCreate(&o.stream2));
            for (auto &e : o.ev) HIP_TRY(hipEventCreate(&e));
            for (auto &e : o.evk) HIP_TRY(hipEventCreate(&e));
            HIP_TRY(hipEventCreateWithFlags(&o.ev_fork, hipEventDisableTiming));
            HIP_TRY(hipEventCreateWithFlags(&o.ev_join, hipEventDisableTiming));
        }
        b->stream = o.stream; b->pooled_stream2 = o.stream2; b->pooled_fork = o.ev_fork; b->pooled_join = o.ev_join;
        for (int k = 0; k < 3; ++k) b->ev[k] = o.ev[k];
        for (int k = 0; k < 7; ++k) b->evk[k] = o.evk[k];
        if (b->n_tiled > 0 && b->n_ring + b->n_wide > 0) { b->stream2 = o.stream2; b->ev_fork = o.ev_fork; b->ev_join = o.ev_join; }
    }
    HIP_TRY(hipMemcpyAsync(base, stage.data(), in_bytes, hipMemcpyHostToDevice, b->stream));
    HIP_TRY(hipStreamSynchronize(b->stream));
    if (verbose)
        std::fprintf(stderr, "pagan_dp: create: plan %.1f ms, hipMalloc of %.0f MB %.1f ms, staging %.0f MB %.1f ms, upload %.1f ms\n",
                     1e3 * (tc1 - tc0), b->arena.size / 1048576.0, 1e3 * (tc2 - tc1), in_bytes / 1048576.0, 1e3 * (tc3 - tc2),
                     1e3 * (now() - tc3));
    guard.b = nullptr;
    *out = b;
    return PAGAN_OK;
}

int pagan_batch_run(pagan_batch *b) {
    if (!b) return PAGAN_E_ARG;
    HIP_TRY(hipSetDevice(b->device));
    if (b->d_guards) {
        // (on the batch's stream, ahead of everything the run launches there; the tiled jobs' stream waits for an event of this one)
        const int init[2] = {0, 0x7fffffff};
        HIP_TRY(hipMemcpyAsync(b->d_canary, init, sizeof init, hipMemcpyHostToDevice, b->stream));
        hipLaunchKernelGGL(pg_canary, dim3(((int)b->guards.size() + 255) / 256), dim3(256), 0, b->stream, b->arena.dev, b->d_guards, (int)b->guards.size(), (int *)nullptr, b->canary_word);
    }
    HIP_TRY(hipEventRecord(b->ev[0], b->stream));
    int rc = launch_fill(b);
    if (rc != PAGAN_OK) return rc;
    HIP_TRY(hipEventRecord(b->ev[1], b->stream));
    if (b->poke[0] >= 0 && b->poke[0] < b->n) {
        hipLaunchKernelGGL(pg_debug_poke_bp, dim3(1), dim3(64), 0, b->stream, b->d_jobs, b->poke[0], b->poke[1], b->poke[2], b->poke[3], (unsigned)b->poke[4]);
        b->poke[0] = -1;
    }
    {
        // (pg_fill_tiles_flow's give-up word sits behind its per-diagonal counters and per-tile flags)
        const bool flow = b->tile_off.size() > 1 && b->tiles_flow;
        const int *gave_up = flow ? b->d_flow + 1 + ((int)b->tile_off.size() - 1) + b->tile_off.back() : nullptr;
        hipLaunchKernelGGL(pg_end_corner, dim3(b->n), dim3(64), 0, b->stream, b->d_jobs, gave_up);
    }
    if (b->max_bound > 0 && b->max_entries > 0)
        hipLaunchKernelGGL(pg_trace_spec, dim3((b->max_entries + 127) / 128, b->n), dim3(128), 0, b->stream, b->d_jobs);
    hipLaunchKernelGGL(pg_trace_compose, dim3(b->n), dim3(64), 0, b->stream, b->d_jobs);
    if (b->max_bound > 0)
        hipLaunchKernelGGL(pg_trace_emit, dim3((2 * b->max_bound + 8 + 63) / 64, b->n), dim3(64), 0, b->stream, b->d_jobs);
    // every visited cell re-evaluated from the stored scores (always on: a back-pointer written from a score that had
    // not landed yet would otherwise be a valid-looking pointer to the wrong cell)
    if (b->max_path > 0)
        hipLaunchKernelGGL(pg_trace_check, dim3((b->max_path + 255) / 256, b->n), dim3(256), 0, b->stream, b->d_jobs, b->flags & 0xffu);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(b->ev[2], b->stream));
    if (b->d_guards)
        hipLaunchKernelGGL(pg_canary, dim3(((int)b->guards.size() + 255) / 256), dim3(256), 0, b->stream, b->arena.dev, b->d_guards, (int)b->guards.size(), b->d_canary, b->canary_word);
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
    HIP_TRY(hipStreamSynchronize(b->stream));
    return canary_verdict(b);
}

int pagan_batch_last_ms(pagan_batch *b, double ms[2]) {
    if (!b || !b->ran) return PAGAN_E_ARG;
    HIP_TRY(hipEventSynchronize(b->ev[2]));
    float a = 0, c = 0;
    HIP_TRY(hipEventElapsedTime(&a, b->ev[0], b->ev[1]));
    HIP_TRY(hipEventElapsedTime(&c, b->ev[1], b->ev[2]));
    ms[0] = a; ms[1] = c;
    return PAGAN_OK;
}

// ms[0] banded fill kernel (pg_fill_pipe / pg_fill_ring), ms[1] pg_backptr, ms[2] tiled fill, ms[3] HBM wavefront fill (from
// the end of whatever ran before it on the stream), ms[4] end corner + traceback, ms[5] the whole fill; -1: not launched
int pagan_batch_last_ms_detail(pagan_batch *b, double ms[6]) {
    if (!b || !b->ran) return PAGAN_E_ARG;
    HIP_TRY(hipEventSynchronize(b->ev[2]));
    auto span = [&](hipEvent_t a, hipEvent_t c, bool ok) -> double {
        float t = 0;
        if (!ok || hipEventElapsedTime(&t, a, c) != hipSuccess) return -1.0;
        return t;
    };
    ms[0] = span(b->evk[0], b->evk[1], b->evk_set[0] && b->evk_set[1]);
    if (ms[0] < 0 && b->evk_set[0]) ms[0] = span(b->evk[0], b->ev[1], true);           // (the ring kernel: no pass behind it)
    ms[1] = span(b->evk[1], b->evk[2], b->evk_set[1] && b->evk_set[2]);
    {   // (+ the pass over the tiled jobs, which runs behind the tiled fill on its stream)
        const double t2 = span(b->evk[4], b->evk[6], b->evk_set[4] && b->evk_set[6]);
        if (t2 >= 0) ms[1] = (ms[1] < 0 ? 0.0 : ms[1]) + t2;
    }
    ms[2] = span(b->evk[3], b->evk[4], b->evk_set[3] && b->evk_set[4]);
    ms[3] = b->evk_set[5] ? span(b->evk_set[2] ? b->evk[2] : (b->evk_set[1] ? b->evk[1] : b->ev[0]), b->evk[5], true) : -1.0;
    ms[4] = span(b->ev[1], b->ev[2], true);
    ms[5] = span(b->ev[0], b->ev[1], true);
    return PAGAN_OK;
}

int64_t pagan_batch_cells(const pagan_batch *b) { return b ? b->cells : 0; }

int pagan_batch_fetch(pagan_batch *b, pagan_result *out) {
    if (!b || !out || !b->ran) return PAGAN_E_ARG;
    HIP_TRY(hipStreamSynchronize(b->stream));
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
            for (int k = 0; k < b->n; ++k) HIP_TRY(hipMemsetAsync(b->dj[k].fill_status, 0, sizeof(int), b->stream));
        // A strip that found the strip above on another XCD gave up (dp_pipe.hip, strip_feeder: tag 11): the strips' launch
        // once more with nothing dispatched beside it
        bool strips_again = false;
        for (int k = 0; k < b->n && !b->strips_alone; ++k) {
            const int st = *reinterpret_cast<const int *>(ends.data() + kEndStride * (size_t)k);
            if (!b->jobs[k].strips.empty() && (st & 0x40000000) && (st & PG_FILL_OTHER_XCD)) strips_again = true;
        }
        if (strips_again) {
            b->strips_alone = true;
            for (int k = 0; k < b->n; ++k)
                if (!b->jobs[k].strips.empty()) HIP_TRY(hipMemsetAsync(b->dj[k].fill_status, 0, sizeof(int), b->stream));
            again = true;
        }
        const char *re = std::getenv("PAGAN_DP_RERUN");
        if (again && !(re && std::strcmp(re, "0") == 0)) {             // (once per fetch; the batch stays without followers)
            if (std::getenv("PAGAN_DP_VERBOSE"))
                std::fprintf(stderr, strips_again ? "pagan_dp: a row strip found the strip above on another XCD: running the batch again, the strips alone\n"
                                     : (score_again ? "pagan_dp: score check failed (a stored score is not what its predecessors give): running the batch again without follower workgroups\n"
                                                    : "pagan_dp: path check failed: running the batch again without follower workgroups\n"));
            if (!strips_again) b->no_follow = true;
            ++b->reruns;
            int rc = pagan_batch_run(b);
            if (rc != PAGAN_OK) return rc;
            HIP_TRY(hipStreamSynchronize(b->stream));
            pagan_batch_last_ms(b, ms);
            HIP_TRY(hipMemcpy(ends.data(), b->arena.dev + b->end_off[0], ends.size(), hipMemcpyDeviceToHost));
        }
    }
    for (int k = 0; k < b->n; ++k) {
        const int st = *reinterpret_cast<const int *>(ends.data() + kEndStride * (size_t)k);
        if (b->strips_alone && !b->jobs[k].strips.empty() && (st & 0x40000000) && (st & PG_FILL_OTHER_XCD)) b->strip_xcd_failure = true;
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
            rcs[k] = replay(orig, f.endcell, f.endscore, f.trace.data(), &out[k]);
            out[k].fill_ms = ms[0];
            out[k].trace_ms = ms[1];
            return;
        }
        rcs[k] = replay(b->jobs[k], got[k].endcell, got[k].endscore, got[k].trace.data(), &out[k]);
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
    HIP_TRY(hipMemsetAsync(b->arena.dev + b->out_begin, 0xFF, b->arena.size - b->out_begin, b->stream));
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
    HIP_TRY(hipStreamSynchronize(b->stream));
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
    HIP_TRY(hipStreamSynchronize(b->stream));
    HIP_TRY(hipMemcpy(dst, b->dj[k].sc, sizeof(double) * (size_t)count, hipMemcpyDeviceToHost));
    return PAGAN_OK;
}

// Diagnostic: job k's back-pointer array, [cells][3] packed words (dp_device.h) in diagonal-major order.
int pagan_batch_debug_backptrs(pagan_batch *b, int32_t k, uint32_t *dst, int64_t count) {
    if (!b || k < 0 || k >= b->n || !dst || count > 3 * b->jobs[k].dx.cells) return PAGAN_E_ARG;
    HIP_TRY(hipStreamSynchronize(b->stream));
    HIP_TRY(hipMemcpy(dst, b->dj[k].bp, sizeof(uint32_t) * (size_t)count, hipMemcpyDeviceToHost));
    return PAGAN_OK;
}

// Diagnostic: raw copy of job k's trace buffer (used by tools/ with a -DPG_STAMPS build).
int pagan_batch_debug_trace(pagan_batch *b, int32_t k, void *dst, int64_t bytes) {
    if (!b || k < 0 || k >= b->n || !dst) return PAGAN_E_ARG;
    HIP_TRY(hipStreamSynchronize(b->stream));
    HIP_TRY(hipMemcpy(dst, b->arena.dev + b->trace_off[k], (size_t)bytes, hipMemcpyDeviceToHost));
    return PAGAN_OK;
}

// Diagnostic: how job k's last traceback was cut (pg_trace_compose's output; tests/trace_plan.py predicts it).  A download only.
int pagan_batch_debug_segments(pagan_batch *b, int32_t k, int32_t info[4], int32_t *segs, int64_t cap) {
    if (!b || k < 0 || k >= b->n || !info || cap < 0 || (cap > 0 && !segs) || !b->ran) return PAGAN_E_ARG;
    HIP_TRY(hipStreamSynchronize(b->stream));
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
    if (b->stream) {
        (void)hipStreamSynchronize(b->stream);
        if (b->pooled_stream2) (void)hipStreamSynchronize(b->pooled_stream2);
        GpuObjs o;
        o.stream = b->stream; o.stream2 = b->pooled_stream2; o.ev_fork = b->pooled_fork; o.ev_join = b->pooled_join;
        for (int k = 0; k < 3; ++k) o.ev[k] = b->ev[k];
        for (int k = 0; k < 7; ++k) o.evk[k] = b->evk[k];
        gpu_pool.give(b->device, o);
    }
    if (b->arena.dev) arena_pool.give(b->device, b->arena.dev, b->arena.cap);
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

int pagan_dp_align_batch(int32_t n, const pagan_job *jobs, const pagan_opts *opts, pagan_result *out) {
    if (!out || n < 0) return PAGAN_E_ARG;
    for (int k = 0; k < n; ++k) std::memset(&out[k], 0, sizeof(pagan_result));
    pagan_batch *b = nullptr;
    const bool verbose = std::getenv("PAGAN_DP_VERBOSE") != nullptr;
    auto now = [] { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    const double t0 = now();
    int rc = pagan_batch_create(n, jobs, opts, &b);
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
    const bool no_strips_now = rc == PAGAN_E_INTERNAL && b->strip_xcd_failure && !tl_no_strips;
    pagan_batch_destroy(b);
    if (no_strips_now) {
        if (verbose) std::fprintf(stderr, "pagan_dp: the strips alone met another XCD again: the batch once more with its wide jobs on the tiled kernel\n");
        tl_no_strips = true;
        rc = pagan_dp_align_batch(n, jobs, opts, out);
        tl_no_strips = false;
        return rc;
    }
    if (verbose)
        std::fprintf(stderr, "pagan_dp: batch of %d: create %.1f ms, kernels %.1f ms, fetch+replay %.1f ms, destroy %.1f ms\n", n,
                     1e3 * (t1 - t0), 1e3 * (t2 - t1), 1e3 * (t3 - t2), 1e3 * (now() - t3));
    return rc;
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
    arena_pool.clear(-1);
    gpu_pool.release();
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
