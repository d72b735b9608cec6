// dp_plan.cpp -- the aligner's host-only planning behind dp_abi.hip (dp_plan.h): the environment switches, validation, the
// band's per-anti-diagonal index, the plan of the banded kernel (classes, far histories, wave schedule, descriptor words), row
// strips and tiles of the wide jobs, the route of every job, dead-site compaction, and the turn of the device's list of
// visited path cells into the reference's path (skip columns + used edges, Viterbi_alignment::backtrack_new_path,
// src/main/viterbi_alignment.cpp:1038-1189).  No HIP here: all of it runs without a device, and the host-only
// pagan_dp_debug_* exports at the end let the tests see it.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <unordered_map>
#include <vector>

#include "dp_plan.h"

// limits of the LDS-staged kernel (dp_kernels.hip: RW site window, EC edge ring)
#define PG_RING_MAX_WIDTH 256
#define PG_RING_SITE_SPAN 576
#define PG_RING_EDGE_CAP 2048
// limits of the register-wavefront kernel: PG_PIPE_* in dp_device.h, shared with dp_pipe.hip

namespace pgplan {

// The one place the environment is read.  (Per call, not once per process: the tests switch the variables.)
DpSwitches DpSwitches::read() {
    auto env = [](const char *name) { return std::getenv(name); };
    auto is = [&](const char *name, const char *value) { const char *e = env(name); return e && std::strcmp(e, value) == 0; };
    DpSwitches s;
    s.fill = is("PAGAN_DP_FILL", "ring") ? FILL_RING : (is("PAGAN_DP_FILL", "tiles") ? FILL_TILES : FILL_PIPE);
    s.bp = is("PAGAN_DP_BP", "verify") ? 2 : (is("PAGAN_DP_BP", "fill") ? 0 : 1);
    if (const char *e = env("PAGAN_DP_DEBUG_FLAGS")) s.debug_flags = (uint32_t)std::strtoul(e, nullptr, 0) & 0xff00u;
    if (const char *e = env("PAGAN_DP_WIDE")) s.wide = std::strcmp(e, "strips") == 0 ? WIDE_STRIPS : (std::strcmp(e, "wavefront") == 0 ? WIDE_WAVEFRONT : WIDE_TILES);
    s.force_global_wavefront = env("PAGAN_DP_FORCE_GLOBAL_WAVEFRONT") != nullptr;
    s.compact = !is("PAGAN_DP_COMPACT", "0");
    if (const char *e = env("PAGAN_DP_STRIP_SPREAD")) s.strip_spread = std::atoi(e) != 0;
    if (const char *e = env("PAGAN_DP_STRIP_STATES")) s.strip_states = std::atoi(e);
    if (const char *e = env("PAGAN_DP_STRIP_SITES")) s.strip_sites = std::atoi(e);
    s.strip_term = env("PAGAN_DP_STRIP_TERM") != nullptr;
    s.tiles = is("PAGAN_DP_TILES", "watermark") ? TILES_WATERMARK : (is("PAGAN_DP_TILES", "nolag") ? TILES_NOLAG : (is("PAGAN_DP_TILES", "launches") ? TILES_LAUNCHES : TILES_FLOW));
    if (const char *e = env("PAGAN_DP_CANARY")) if (std::strcmp(e, "0") != 0) {
        s.canary = true;
        if (e[0] == '0' && e[1] == 'x') s.canary_word = (unsigned)std::strtoul(e, nullptr, 16);
    }
    s.wide7 = !is("PAGAN_DP_WIDE7", "0");
    s.hist = is("PAGAN_DP_HIST", "0") ? HIST_OFF : (is("PAGAN_DP_HIST", "narrow") ? HIST_NARROW : HIST_ON);
    s.three = !is("PAGAN_DP_THREE", "0");
    // a diagonal fewer than this behind a wide one is a general step (classify_diagonals); =reach: REACH, as before round 5 (A/B switch)
    s.after_wide = is("PAGAN_DP_AFTER_WIDE", "reach") ? PG_PIPE_REACH : 3;
    if (const char *e = env("PAGAN_DP_PLAN_THREADS")) s.plan_threads = std::max(1, std::atoi(e));
    s.score_check = is("PAGAN_DP_SCORE_CHECK", "0") ? CHECK_OFF : (is("PAGAN_DP_SCORE_CHECK", "all") ? CHECK_ALL : CHECK_DEFAULT);
    s.follow = !is("PAGAN_DP_FOLLOW", "0");
    s.rerun = !is("PAGAN_DP_RERUN", "0");
    s.verbose = env("PAGAN_DP_VERBOSE") != nullptr;
    static const bool prof = env("PAGAN_DP_PLAN_PROFILE") != nullptr;
    s.plan_profile = prof;
    return s;
}

static double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
Lap::Lap(const char *prefix_, bool on_) : prefix(prefix_), on(on_), t_last(on_ ? now_ms() : 0.0) {}
void Lap::operator()(const char *what) {
    if (!on) return;
    const double t = now_ms();
    std::fprintf(stderr, "%s%s %.2f ms\n", prefix, what, t - t_last);
    t_last = t;
}

namespace {

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
                   const SiteFeat &fl, const SiteFeat &fr, const DpSwitches &sw, FarPlan *out) {
    const int nd = Lx + Ly - 1;
    out->hfL.assign(Lx, 0); out->hfR.assign(Ly, 0); out->hbit.assign(nd, 0);
    out->servedL.assign(Lx, 0); out->servedR.assign(Ly, 0);
    out->n_served = out->n_hard = 0;
    if (sw.hist == DpSwitches::HIST_OFF) return;      // PAGAN_DP_HIST=0, A/B switch: every far site as before
    // diagonals that do not run in the hand-scheduled loop whatever the sites are (classify_diagonals has the rules)
    std::vector<int> slow(nd + 1, 0);
    {
        const int after_wide = sw.after_wide;
        // (round 5) the wide runs and the general steps behind them append to the history lines like the loop does (wide_run7,
        // wide_run, the kernel's general step): an interval may cross them; only class 5 diagonals -- and the steps behind THOSE --
        // write no history.  PAGAN_DP_HIST=narrow: as before (A/B).
        const bool hist_wide = sw.hist != DpSwitches::HIST_NARROW;
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
                        const DiagIndex &dx, bool inwave, const DpSwitches &sw, std::vector<uint8_t> *out, std::vector<int> *lead_req,
                        std::vector<uint8_t> *ring2 = nullptr, int threads = 1, FarPlan *far_plan = nullptr) {
    const int nd = Lx + Ly - 1;
    Lap lap("pagan_dp:   classify: ", sw.plan_profile);
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
    if (far_plan && inwave) plan_far_hist(L, R, Lx, Ly, rb, dx, fl, fr, sw, far_plan);
    else { fp.servedL.assign(Lx, 0); fp.servedR.assign(Ly, 0); fp.hbit.assign(nd, 0); }
    lap("far histories");
    // three-edge sites in the lanes (hand-scheduled loop, with a plan that can carry the per-diagonal bit)
    const bool three_ok = far_plan && inwave && sw.three;
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
    const int after_wide = sw.after_wide;
    par_ranges(nd, threads, [&](int d_first, int d_last) {
        for (int d = d_first; d < d_last; ++d) {
            const int run = run_at[d];
            const int lo = dx.imin[d], hi = dx.imax[d];
            uint8_t c;
            // Behind a wide diagonal (the ring's memory was the wide ring): after_wide - 1 = two general steps -- the first leaves the
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
                 std::vector<StripPlan> *out, int max_sites, int *sites_seen, bool big_table, const DpSwitches &sw) {
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
    const bool term_cxx = sw.strip_term;
    // three-edge sites in the lanes (round 5; classify_diagonals has the rules): small model tables only -- the hand-scheduled loop
    const bool three_ok = !big_table && sw.three;
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
} // namespace

// ---- dead sites ----------------------------------------------------------------------------------------------------
// A site without bwd edges (other than the start site) -- or with bwd edges from such sites only -- has no live
// predecessor: every cell of its row / column is -inf in all three states, nothing can leave it, and no path visits it (the path SKIPS it: insert_preexisting_gap,
// viterbi_alignment.h:146-193, restated in replay()).  High in a deep tree such sites are many (root of 512 x 10 kb: 44 %
// of each sequence), so the alignment is run on the COMPACTED graphs -- dead sites removed, the edges that start at one
// dropped (their candidates are -inf), the band re-indexed -- and the device's path is mapped back to the caller's site
// numbers and edge-list positions before replay() turns it into columns and used edges.  Scores, path and used edges are
// the ones of the full matrices; `cells` stays the caller's count.  PAGAN_DP_COMPACT=0 switches it off.
void CompactSide::build(const pagan_graph *o) {
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

// The caller's band over the compacted matrices: row t is the caller's row l.keep[t]; its interval keeps the first / last
// kept column inside the caller's interval (empty where none is).  rb0: the caller's band, clamped (RowBand).
static void compact_band(const RowBand &rb0, const CompactSide &l, const CompactSide &r, int nr, std::vector<int> *up, std::vector<int> *lo) {
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


Route route_of(const HostJob &hj, int n_states, const DpSwitches &sw) {
    // (PAGAN_DP_FORCE_GLOBAL_WAVEFRONT, and PAGAN_DP_WIDE=wavefront for the wide jobs: the one-workgroup HBM wavefront, A/B switches)
    if (hj.ring_ok && !sw.force_global_wavefront) return n_states <= 16 ? PIPE_SMALL : PIPE_BIG;     // model tables of <= 16 states (DNA: 15) are cached in LDS
    const bool use_tiles = !sw.force_global_wavefront && sw.wide != DpSwitches::WIDE_WAVEFRONT;
    if (use_tiles && !hj.strips.empty()) return STRIPS;
    if (use_tiles && !hj.tiles.empty()) return TILES;
    return WAVEFRONT;
}

int validate_job(const pagan_job &jb, HostJob *hj, const DpSwitches &sw, bool allow_strips, int threads) {
    if (!jb.left || !jb.right || !jb.model) return PAGAN_E_ARG;
    int rc;
    RowBand rb;
    const bool use_pipe = sw.fill != DpSwitches::FILL_RING;
    // (PAGAN_DP_PLAN_PROFILE: milliseconds per phase of the plan of one job, on stderr)
    Lap lap("pagan_dp: plan ", sw.plan_profile);
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
    if ((rc = rb.build(hj->Lx, hj->Ly, jb.band)) != PAGAN_OK) return rc;
    lap("row band");
    hj->dx.build(hj->Lx, hj->Ly, rb);
    if (hj->dx.cells != rb.cells()) return PAGAN_E_INTERNAL;
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
    if (sw.fill == DpSwitches::FILL_TILES) narrow = false;   // PAGAN_DP_FILL=tiles, A/B switch
    if (use_pipe) {
        hj->ring_ok = narrow && edges_fit_ring(jb.left, hj->Lx, PG_PIPE_EDGE_CAP, PG_PIPE_SITE_EDGES) &&
                      edges_fit_ring(jb.right, hj->Ly, PG_PIPE_EDGE_CAP, PG_PIPE_SITE_EDGES);
        if (hj->ring_ok) {
            lap("boundaries, edge windows");
            FarPlan fp;
            classify_diagonals(jb.left, jb.right, hj->Lx, hj->Ly, rb, hj->dx, jb.model->n_states * jb.model->n_states <= 256, sw,
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
        list_tiles(hj->Lx, rb, &hj->tiles);
    // Row strips on the banded kernel (dp_pipe.hip, strip_feeder): a wide job whose model table fits LDS and whose edge lists
    // fit the kernel's windows, unless a diagonal of a strip would hold more multi-edge sites than the kernel's assist waves
    // keep in their lanes (plan_strips).  PAGAN_DP_WIDE=tiles keeps every wide job on the tiled kernel (A/B switch).
    {
        const bool want = sw.wide == DpSwitches::WIDE_STRIPS && allow_strips;
        // Models whose table does not fit LDS (S > 16) run as strips only on request (PAGAN_DP_STRIP_STATES = the largest model that
        // does): correct (tests/test_strips_gpu.py) and slower than the tiles from the third level of a tree on -- the assist
        // waves gather a model score for every cell and stage every multi-edge cell with their general code (cfg3: 23.4 -> 57.8 ms).
        const int max_states = sw.strip_states;
        if (want && use_pipe && !hj->ring_ok && !neg0 && !hj->tiles.empty() && jb.model->n_states <= max_states &&
            hj->Lx >= 2 && hj->Ly >= 2 &&
            edges_fit_ring(jb.left, hj->Lx, PG_PIPE_EDGE_CAP, PG_PIPE_SITE_EDGES) && edges_fit_ring(jb.right, hj->Ly, PG_PIPE_EDGE_CAP, PG_PIPE_SITE_EDGES))
        {
            int seen = 0;
            const bool ok = plan_strips(jb.left, jb.right, hj->Lx, hj->Ly, rb, hj->dx, &hj->strips, sw.strip_sites, &seen,
                                        jb.model->n_states * jb.model->n_states > 256, sw);
            if (sw.verbose)
                std::fprintf(stderr, "pagan_dp: wide job %d x %d: at most %d multi-edge sites on a strip's diagonal: %s\n", hj->Lx, hj->Ly, seen,
                             ok ? "row strips" : "tiles");
        }
    }
    hj->route = route_of(*hj, jb.model->n_states, sw);
    return PAGAN_OK;
}

// (dp_plan.h) pure host code: pagan_batch_create writes the words straight into its staging buffer, pagan_dp_debug_descriptors
// into the caller's array.
void pack_pipe_descriptors(const HostJob &hj, int n_states, const DpSwitches &sw, int *packed) {
    std::memset(packed + 8 * hj.dx.imin.size(), 0, 8 * sizeof(int));                             // the entry of padding
    unsigned mask = 0;             // bit a: diagonal t-a was computed by the lanes (class <= 3), a = 1 .. REACH-1
    // hop[t]: how many of its own diagonals (t + PNA, t + 2 PNA, ...) an assist wave may skip after t before the
    // next one with work for it (a multi-edge cell, or -- model table too large for LDS -- any interior diagonal);
    // 12 bits, saturating: it looks again after a saturated hop
    const size_t ndg = hj.dx.imin.size();
    const bool big_table = n_states * n_states > 256;
    // wide runs (consecutive class 4 diagonals): does any diagonal of the run exceed PG_PIPE_WINDOW_A cells?  (bit 4 of a class
    // 4 diagonal's word: wide_run takes the wide-ring geometry with more positions and fewer rows then.)  Bit 19: the run has
    // at least PG_PIPE_ASSIST diagonals (small tables) -- every assist wave meets one of them, and the run is wide_run7's:
    // the assist waves take rows of their own.  PAGAN_DP_WIDE7=0: every run stays with the four compute waves (A/B switch)
    const bool wide7_on = sw.wide7;
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
}


// Dead sites out of one job (see CompactJob): fills `cj` and points `eff` at the compacted graphs / band when the job
// qualifies (5 % dead sites or more, nothing validate_job would refuse).
void compact_job(const pagan_job &jb, bool allow, CompactJob *cjp, pagan_job *eff) {
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

// tile launches: launch t takes the tiles with row + column = t of every tiled job
void build_tile_list(const std::vector<HostJob> &jobs, const std::vector<int> &which_tiled, std::vector<int> *tile_list_out,
                     std::vector<int> *tile_off_out, bool *water) {
    std::vector<int> &tile_list = *tile_list_out, &tile_off = *tile_off_out;
    if (which_tiled.empty()) return;
    int T = 0;
    for (int k : which_tiled) {
        const std::vector<int> &tl = jobs[k].tiles;
        for (size_t q = 0; q < tl.size(); q += 2) T = std::max(T, tl[q] + tl[q + 1] + 1);
    }
    tile_off.assign(T + 1, 0);
    for (int k : which_tiled) {
        const std::vector<int> &tl = jobs[k].tiles;
        for (size_t q = 0; q < tl.size(); q += 2) ++tile_off[tl[q] + tl[q + 1] + 1];
    }
    for (int t = 0; t < T; ++t) tile_off[t + 1] += tile_off[t];
    const size_t N = (size_t)tile_off[T];
    tile_list.assign(4 * N + 4 + 2 * N + (size_t)T + 1, 0);
    std::vector<int> cur(tile_off.begin(), tile_off.end() - 1);
    std::unordered_map<uint64_t, int> where;               // (job, tile row, tile column) -> position in the list
    where.reserve(2 * N);
    auto key = [](int k, int a, int bb) { return ((uint64_t)(uint32_t)k << 40) | ((uint64_t)(uint32_t)a << 20) | (uint64_t)(uint32_t)bb; };
    for (int k : which_tiled) {
        const std::vector<int> &tl = jobs[k].tiles;
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
    for (int t = 0; t <= T; ++t) tile_list[4 * N + 4 + 2 * N + (size_t)t] = tile_off[t];
    // The neighbour flags alone order a tile behind everything it can read only if the job's tiles form a staircase
    // (dp_tiles.hip): every tile row a contiguous run of columns, first and last column never falling from one row to
    // the next, no empty row between two rows, consecutive rows touching.
    for (int k : which_tiled) {
        const bool stair = tiles_staircase(jobs[k].tiles);
        if (!stair) *water = true;
    }
}

// Row strips: every strip a device job of its own behind the batch's n; the strips of a job at workgroup indices of one
// residue mod 8 (one XCD: a strip reads what the strip above stored from that XCD's L2), in order
void order_strips(const std::vector<HostJob> &jobs, const std::vector<pagan_job> &eff, const std::vector<int> &which_striped, int n,
                  bool spread, std::vector<std::pair<int, int>> *sdev_out, std::vector<int> *swhich_out, int grid[2]) {
    std::vector<std::pair<int, int>> &sdev = *sdev_out;
    std::vector<int> &swhich = *swhich_out;
    // a job to the XCD with the least work so far (largest jobs first); inside an XCD's list the strips of its jobs by
    // first diagonal: workgroups are dispatched in index order and a strip holds its compute unit while it waits for the
    // strip above, so what is resident should be what can run -- the fronts of all the XCD's jobs, not one job's whole
    // chain.  (A job's strips stay in order: their first diagonals grow.)  A strip's device job is found through `where`.
    // device jobs of the strips: job-major (a strip finds the strip above in the entry before its own)
    std::unordered_map<long long, int> where;
    for (int k : which_striped)
        for (size_t q = 0; q < jobs[k].strips.size(); ++q) {
            where[((long long)k << 20) | (long long)q] = n + (int)sdev.size();
            sdev.push_back({k, (int)q});
        }
    // two dispatches: the jobs whose model table fits LDS (pg_fill_pipe<true, true>), then the others (<false, true>)
    for (int big = 0; big < 2; ++big) {
        std::vector<int> by_size;
        for (int k : which_striped) if ((eff[k].model->n_states * eff[k].model->n_states > 256) == (big == 1)) by_size.push_back(k);
        std::stable_sort(by_size.begin(), by_size.end(), [&](int a, int c) { return jobs[a].dx.cells > jobs[c].dx.cells; });
        long long lane_cells[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        std::vector<std::vector<std::pair<int, int>>> lane_strips(8);          // (job, strip)
        for (int k : by_size) {
            int lane = 0;
            for (int x = 1; x < 8; ++x) if (lane_cells[x] < lane_cells[lane]) lane = x;
            lane_cells[lane] += jobs[k].dx.cells;
            for (size_t q = 0; q < jobs[k].strips.size(); ++q) lane_strips[lane].push_back({k, (int)q});
        }
        const size_t first = swhich.size();                          // (a multiple of 8)
        if (spread) {
            // PAGAN_DP_STRIP_SPREAD (the default, round 5): a job's strips on ANY XCD -- they store their scores through to
            // memory and read the strip above's with sc1 loads (dp_pipe.hip, store_scores / strip_feeder), so a single wide job
            // (the root of a tree) has the whole chip, not one XCD's 32 units.  All strips of the launch in the order of their
            // first diagonals: the order they can start in (a job's own strips stay in order: their first diagonals grow).
            std::vector<std::pair<int, int>> all;
            for (int lane = 0; lane < 8; ++lane) all.insert(all.end(), lane_strips[lane].begin(), lane_strips[lane].end());
            std::stable_sort(all.begin(), all.end(), [&](const std::pair<int, int> &a, const std::pair<int, int> &c) {
                const int da = jobs[a.first].strips[a.second].d0, dc = jobs[c.first].strips[c.second].d0;
                return da != dc ? da < dc : (a.first != c.first ? a.first < c.first : a.second < c.second); });
            for (const auto &js : all) swhich.push_back(where[((long long)js.first << 20) | (long long)js.second]);
            while (swhich.size() % 8) swhich.push_back(-1);
        } else
        for (int lane = 0; lane < 8; ++lane) {
            auto &ls = lane_strips[lane];
            std::stable_sort(ls.begin(), ls.end(), [&](const std::pair<int, int> &a, const std::pair<int, int> &c) {
                return jobs[a.first].strips[a.second].d0 < jobs[c.first].strips[c.second].d0; });
            for (size_t pos = 0; pos < ls.size(); ++pos) {
                const size_t at = first + 8 * pos + lane;
                if (swhich.size() <= at) swhich.resize(first + ((at - first) / 8 + 1) * 8, -1);
                swhich[at] = where[((long long)ls[pos].first << 20) | (long long)ls[pos].second];
            }
        }
        grid[big] = (int)(swhich.size() - first);
    }
}

// Host side of backtrack_new_path (VA:1038-1189): the device reports the visited cells
// end -> start; this re-inserts the skipped child sites (insert_preexisting_gap,
// viterbi_alignment.h:146-193), applies insert_new_path_pointer's `i>0 || j>0` rule
// (viterbi_alignment.h:196-200), marks the child edges the path used, and numbers the
// columns the way create_ancestral_sequence consumes them (basic_alignment.cpp:73-171).
int replay(const HostJob &hj, const int *endcell, double endscore, const int *trace, bool verbose, pagan_result *out) {
    const pagan_graph *L = hj.L, *R = hj.R;
    const int Lx = hj.Lx, Ly = hj.Ly;
    std::memset(out, 0, sizeof(*out));
    out->cells = hj.dx.cells;
    out->score = endscore;
    // nothing the device wrote is used as an index before it has been checked against the graphs
    if (endcell[0] != 0 && endcell[0] != 1) {
        if (verbose) std::fprintf(stderr, "pagan_dp: device status %d\n", endcell[0]);
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

} // namespace pgplan

using namespace pgplan;

// The traceback's host half for callers outside this file (dp_fb.hip: a sampled path has the same shape as a
// Viterbi path): endcell / trace in the device's format (dp_device.h).
int pagan_internal_replay(const pagan_graph *L, const pagan_graph *R, int64_t cells, const int *endcell, double endscore,
                          const int *trace, pagan_result *out) {
    HostJob hj;
    hj.L = L; hj.R = R; hj.Lx = L->n_sites - 1; hj.Ly = R->n_sites - 1;
    hj.dx.cells = cells;
    return replay(hj, endcell, endscore, trace, DpSwitches::read().verbose, out);
}

extern "C" {

// Host-only: which fill kernel pagan_batch_create would give this job -- its Route: 0 pg_fill_pipe (model table in LDS), 1
// pg_fill_pipe (large table), 2 pg_fill_tiles_flow, 3 pg_fill_wavefront, 4 pg_fill_pipe (row strips) -- after taking its dead sites
// out as the batch does (the batch's own steps: compact_job, validate_job, the route it stores); negative: the error
// validate_job reports.  n_out[0] = 1 when the job is aligned on compacted graphs, n_out[1] = widest diagonal.
int pagan_dp_debug_route(const pagan_graph *left, const pagan_graph *right, const pagan_model *model, const pagan_band *band,
                         int32_t *n_out) {
    pagan_job jb;
    std::memset(&jb, 0, sizeof(jb));
    jb.left = left; jb.right = right; jb.model = model; jb.band = band;
    pagan_job eff = jb;
    CompactJob cj;
    const DpSwitches sw = DpSwitches::read();
    compact_job(jb, sw.compact, &cj, &eff);
    HostJob hj;
    const int rc = validate_job(eff, &hj, sw);
    if (rc != PAGAN_OK) return rc;
    if (n_out) { n_out[0] = cj.on ? 1 : 0; n_out[1] = hj.dx.max_width; }
    return hj.route;
}

// What the host-only exports below open with: both graphs checked, the row band and (dx != nullptr) its diagonal index built.
// expect_nd >= 0: the number of diagonals the caller's arrays were sized for.
static int debug_preface(const pagan_graph *left, const pagan_graph *right, const pagan_band *band, int expect_nd, Lap *lap,
                         int *Lx, int *Ly, RowBand *rb, DiagIndex *dx) {
    int rc;
    if ((rc = check_graph(left)) != PAGAN_OK) return rc;
    if ((rc = check_graph(right)) != PAGAN_OK) return rc;
    *Lx = left->n_sites - 1; *Ly = right->n_sites - 1;
    if (expect_nd >= 0 && expect_nd != *Lx + *Ly - 1) return PAGAN_E_ARG;
    if (lap) (*lap)("checks");
    if ((rc = rb->build(*Lx, *Ly, band)) != PAGAN_OK) return rc;
    if (lap) (*lap)("row band");
    if (dx) dx->build(*Lx, *Ly, *rb);
    if (lap) (*lap)("diagonal index");
    return PAGAN_OK;
}

// Host-only: the per-diagonal classes and the wave schedule pg_fill_pipe would be given for this job
// (what validate_job computes); lets the planner be tested without a device.
int pagan_dp_debug_plan(const pagan_graph *left, const pagan_graph *right, const pagan_band *band, uint8_t *cls_out,
                        int32_t n_cls, int32_t *sched_out, int32_t sched_cap, int32_t *sched_len, int32_t *lead_req_out) {
    if (!left || !right || !cls_out || !sched_out || !sched_len) return PAGAN_E_ARG;
    const DpSwitches sw = DpSwitches::read();
    Lap lap("pagan_dp: plan ", sw.plan_profile);
    int Lx, Ly;
    RowBand rb;
    DiagIndex dx;
    if (const int rc = debug_preface(left, right, band, n_cls, &lap, &Lx, &Ly, &rb, &dx)) return rc;
    std::vector<uint8_t> cls;
    std::vector<int> sched, lead_req;
    const int threads = sw.plan_threads;                        // PAGAN_DP_PLAN_THREADS: the plan over several threads (tests compare with one)
    classify_diagonals(left, right, Lx, Ly, rb, dx, true, sw, &cls, &lead_req, nullptr, threads);      // the plan of a job whose model table fits LDS
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
    int Lx, Ly;
    RowBand rb;
    DiagIndex dx;
    if (const int rc = debug_preface(left, right, band, -1, nullptr, &Lx, &Ly, &rb, &dx)) return rc;
    std::vector<uint8_t> cls;
    std::vector<int> lead_req;
    FarPlan fp;
    classify_diagonals(left, right, Lx, Ly, rb, dx, true, DpSwitches::read(), &cls, &lead_req, nullptr, 1, &fp);
    std::memcpy(hfL, fp.hfL.data(), fp.hfL.size()); std::memcpy(hfR, fp.hfR.data(), fp.hfR.size());
    for (size_t d = 0; d < fp.hbit.size(); ++d) hbit[d] = (uint8_t)(fp.hbit[d] | (fp.tbit.size() > d && fp.tbit[d] ? 2 : 0));     // bit 1: the third pass
    std::memcpy(cls_out, cls.data(), cls.size());
    return fp.n_served;
}

// Host-only: the descriptor words pg_fill_pipe would read for this job (PgDevJob::psc, 8 per diagonal: first row, last row, byte
// offset of the first score (2), class | bit 4 | residency mask with bit 5 | bit 19 | hop, cell offset (2), lead_req) under a
// model of n_states states.  Returns the number of diagonals, 0 for a job the planner does not give to pg_fill_pipe.
int pagan_dp_debug_descriptors(const pagan_graph *left, const pagan_graph *right, const pagan_band *band, int32_t n_states,
                               int32_t *words, int64_t cap) {
    if (!left || !right || !words || n_states <= 0 || cap < 0) return PAGAN_E_ARG;
    const std::vector<float> table((size_t)n_states * n_states, 0.0f);
    pagan_model model;
    std::memset(&model, 0, sizeof(model));
    model.n_states = n_states; model.log_score = table.data();
    pagan_job jb;
    std::memset(&jb, 0, sizeof(jb));
    jb.left = left; jb.right = right; jb.model = &model; jb.band = band;
    HostJob hj;
    const DpSwitches sw = DpSwitches::read();
    const int rc = validate_job(jb, &hj, sw);
    if (rc != PAGAN_OK) return rc;
    if (hj.route != PIPE_SMALL && hj.route != PIPE_BIG) return 0;
    const int64_t nd = (int64_t)hj.cls.size();
    if (8 * nd > cap) return PAGAN_E_ARG;
    std::vector<int> packed(8 * ((size_t)nd + 1));
    pack_pipe_descriptors(hj, n_states, sw, packed.data());
    std::memcpy(words, packed.data(), sizeof(int) * 8 * (size_t)nd);
    return (int)nd;
}

int pagan_dp_debug_strips(const pagan_graph *left, const pagan_graph *right, const pagan_band *band, int32_t max_sites,
                          int32_t *strips, int32_t cap, int64_t *desc_off, int64_t *desc, int64_t desc_cap) {
    if (!left || !right || !strips || !desc_off || !desc || cap < 0 || desc_cap < 0) return PAGAN_E_ARG;
    int Lx, Ly;
    RowBand rb;
    DiagIndex dx;
    if (const int rc = debug_preface(left, right, band, -1, nullptr, &Lx, &Ly, &rb, &dx)) return rc;
    std::vector<StripPlan> plan;
    int seen = 0;
    if (!plan_strips(left, right, Lx, Ly, rb, dx, &plan, max_sites > 0 ? max_sites : (1 << 30), &seen, false, DpSwitches::read())) return 0;
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
    int Lx, Ly;
    RowBand rb;
    if (const int rc = debug_preface(left, right, band, -1, nullptr, &Lx, &Ly, &rb, nullptr)) return rc;
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


} // extern "C"
