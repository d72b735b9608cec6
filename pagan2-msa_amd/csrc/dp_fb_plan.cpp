// dp_fb_plan.cpp -- the forward/backward side's planning, host only (dp_fb_plan.h): the switch table, the plan of one pair, the
// host-only exports that report it, and the size predictor that needs nothing else.
#include "dp_fb_plan.h"

#include <cstdlib>
#include <cstring>

namespace fbplan {

FbSwitches FbSwitches::read() {
    auto env = [](const char *name) { return std::getenv(name); };
    auto off = [&](const char *name) { const char *e = env(name); return e && std::strcmp(e, "0") == 0; };
    auto num = [&](const char *name, int dflt) { const char *e = env(name); return e ? std::atoi(e) : dflt; };
    FbSwitches s;
    s.ring = !off("PAGAN_FB_RING");
    s.ring_min_nd = num("PAGAN_FB_RING_MIN_ND", 256);   // (a step of the ring sweeps is 1 us against the one-workgroup kernels' 2.7: worth it from a few hundred diagonals on)
    s.ring_split = !off("PAGAN_FB_RING_SPLIT");
    s.deep = !off("PAGAN_FB_DEEP");
    s.deep_min_nd = num("PAGAN_FB_DEEP_MIN_ND", 4096);
    if (const char *e = env("PAGAN_FB_BAND_MIN_ND")) s.band_min_nd = std::strcmp(e, "off") == 0 ? 0x7fffffff : std::atoi(e);
    if (const char *e = env("PAGAN_FB_GROUPS")) { s.groups_set = true; s.groups = std::max(1, std::min(FB_MAX_GROUPS, std::atoi(e))); }
    s.slots_x16 = std::max(8, std::min(48, num("PAGAN_FB_SLOTS_X16", 46)));   // 2.9 workgroups per compute unit of the 3 that fit (A/B; 2.5 until round 5)
    s.split = std::max(20, std::min(80, num("PAGAN_FB_SPLIT", 40)));
    s.bwd_first = env("PAGAN_FB_BWD_FIRST") != nullptr;
    s.decode_ring = !off("PAGAN_FB_DECODE_RING");
    s.verbose = env("PAGAN_DP_VERBOSE") != nullptr;
    return s;
}

FwdLists forward_lists(const pagan_graph *g) {
    struct E { int src, dst, eid; float lw; };
    std::vector<E> es;
    es.reserve(g->bwd_off[g->n_sites]);
    for (int s = 0; s < g->n_sites; ++s)
        for (int k = g->bwd_off[s]; k < g->bwd_off[s + 1]; ++k) es.push_back({g->bwd_src[k], s, g->bwd_eid[k], g->bwd_logw[k]});
    std::stable_sort(es.begin(), es.end(), [](const E &a, const E &b) { return a.src != b.src ? a.src < b.src : a.eid < b.eid; });
    FwdLists f;
    f.off.assign(g->n_sites + 1, 0);
    for (const E &e : es) f.off[e.src + 1]++;
    for (int s = 0; s < g->n_sites; ++s) f.off[s + 1] += f.off[s];
    for (const E &e : es) { f.dst.push_back(e.dst); f.lw.push_back(e.lw); }
    return f;
}

int fb_block_for(int width, bool one_workgroup) {
    // the widest diagonal the rungs 64 / 128 / 256 / 512 take (a wider one: 1,024): a row each; 1.5 cells a thread less one
    static const int widest[2][4] = {{64, 128, 256, 512}, {95, 191, 383, 767}};
    int b = 64;
    for (int k = 0; k < 4 && width > widest[one_workgroup ? 1 : 0][k]; ++k) b *= 2;
    return b;
}

namespace {

// initialise_array_corner_bwd (VA:740-854): assignments onto the cells the end corner reads
void fb_corner_init(const pagan_graph *left, const pagan_graph *right, double l_ng, FbPlan *P) {
    const int Lx = P->Lx, Ly = P->Ly;
    P->init_dmin = P->nd;
    auto put_init = [&](int i, int j, int s, double v) {
        const long long a = P->dx.at(i, j);
        if (a < 0) return;
        P->init_dmin = std::min(P->init_dmin, i + j);
        for (size_t k = 0; k < P->init_at.size(); ++k) if (P->init_at[k] == 3 * a + s) { P->init_val[k] = v; return; }   // later assignment wins
        P->init_at.push_back(3 * a + s); P->init_val.push_back(v);
    };
    put_init(Lx - 1, Ly - 1, PAGAN_M_MAT, l_ng);
    const int l0 = left->bwd_off[Lx], l1 = left->bwd_off[Lx + 1], r0 = right->bwd_off[Ly], r1 = right->bwd_off[Ly + 1];
    if (l1 > l0 && r1 > r0)
        for (int k1 = l0; k1 < l1; ++k1)
            for (int k2 = r0; k2 < r1; ++k2)
                put_init(left->bwd_src[k1], right->bwd_src[k2], PAGAN_M_MAT, l_ng + (double)left->bwd_logw[k1] + (double)right->bwd_logw[k2]);
    for (int k1 = l0; k1 < l1; ++k1) put_init(left->bwd_src[k1], Ly - 1, PAGAN_X_MAT, 0.0);
    for (int k2 = r0; k2 < r1; ++k2) put_init(Lx - 1, right->bwd_src[k2], PAGAN_Y_MAT, 0.0);
}

// v[k] := max of v over [k - before, k + after]
void fb_window_max(std::vector<int> &v, int before, int after) {
    const int n = (int)v.size();
    std::vector<int> out(n), dq(n);
    int head = 0, tail = 0, nxt = 0;
    for (int k = 0; k < n; ++k) {
        for (; nxt < n && nxt <= k + after; ++nxt) { while (tail > head && v[dq[tail - 1]] <= v[nxt]) --tail; dq[tail++] = nxt; }
        while (dq[head] < k - before) ++head;
        out[k] = v[dq[head]];
    }
    v.swap(out);
}

// The deep-ring plan.  A diagonal needs B >= its own width and that of the FB_DP_HALO diagonals either side of it (the ring of a
// segment is rebuilt from them at its boundary, in either direction).  Segments: greedy, a segment's B only grows while it is
// shorter than FB_DP_MINSEG diagonals, ends where a wider diagonal comes, and where the next FB_DP_MINSEG diagonals all fit a smaller B.
void fb_deep_plan(const std::vector<int> &rL, const std::vector<int> &rR, const std::vector<int> &sL, const std::vector<int> &sR, FbPlan *P) {
    const int nd = P->nd;
    const DiagIndex &dx = P->dx;
    std::vector<int> need(nd);
    for (int d = 0; d < nd; ++d) need[d] = fb_block_for(dx.imax[d] - dx.imin[d] + 1);
    fb_window_max(need, FB_DP_HALO, FB_DP_HALO);
    std::vector<int> ahead(need);
    fb_window_max(ahead, 0, FB_DP_MINSEG - 1);
    int maxB = 64, minD = FB_DP_CELLS / 64;
    for (int s = 0; s < nd;) {
        int B = need[s], e = s + 1;
        for (; e < nd; ++e) {
            const int nb = need[e];
            if (nb == B) continue;
            if (e - s < FB_DP_MINSEG) { B = std::max(B, nb); continue; }
            if (nb > B || ahead[e] < B) break;
        }
        P->seg_start.push_back(s); P->seg_B.push_back(B);
        maxB = std::max(maxB, B); minD = std::min(minD, FB_DP_CELLS / B);
        s = e;
    }
    P->seg_start.push_back(nd);
    // far cells: a predecessor (forward: reaches rL / rR of the bwd lists) or successor (backward: sL / sR of the fwd lists) D or more diagonals away
    P->dfar.assign(nd, 0);
    long long far_cells = 0; int far_diags = 0;
    for (size_t g = 0; g + 1 < P->seg_start.size(); ++g) {
        const int D = FB_DP_CELLS / P->seg_B[g];
        int any = 0;
        for (int d = P->seg_start[g]; d < P->seg_start[g + 1]; ++d) {
            int f = 0;
            for (int i = dx.imin[d]; i <= dx.imax[d]; ++i) {
                const int j = d - i;
                const int a = i > 0 ? rL[i] : 0, b = j > 0 ? rR[j] : 0;
                if (a >= D || b >= D || (a > 0 && b > 0 && a + b >= D)) { ++far_cells; f |= 1; }
                if (sL[i] >= D || sR[j] >= D || (sL[i] > 0 && sR[j] > 0 && sL[i] + sR[j] >= D)) f |= 2;
            }
            P->dfar[d] = f; any |= f;
            if (f & 1) ++far_diags;
        }
        if (any) P->seg_B[g] |= 1 << 16;
    }
    P->block = std::min(FB_RG_THREADS, 3 * maxB);
    P->info[2] = (int)P->seg_B.size(); P->info[3] = minD;
    P->info[6] = (int)std::min<long long>(far_cells, 0x7fffffff); P->info[7] = far_diags;
}

// a plain sequence: every site has exactly one edge, from the site before it
bool fb_plain(const pagan_graph *g) {
    for (int sidx = 1; sidx < g->n_sites; ++sidx)
        if (g->bwd_off[sidx + 1] - g->bwd_off[sidx] != 1 || g->bwd_src[g->bwd_off[sidx]] != sidx - 1) return false;
    return g->bwd_off[1] == 0;
}
// no cell diagonal without a cell
bool fb_gapless(const DiagIndex &dx, int nd) {
    for (int d = 0; d < nd; ++d) if (dx.imax[d] < dx.imin[d]) return false;
    return true;
}

// Which schedule the pair's sweeps take, and for the deep-ring sweeps their plan: the segments and the diagonals that hold a far cell.
void fb_route(const pagan_graph *left, const pagan_graph *right, bool has_band, const FbSwitches &sw, FbPlan *P) {
    const int Lx = P->Lx, Ly = P->Ly, nd = P->nd, mw = P->dx.max_width;
    const int blocks_x = (Lx + FB_T - 1) / FB_T, blocks_y = (Ly + FB_T - 1) / FB_T;
    const bool both_plain = P->both_plain;
    const bool shape_ok = mw <= FB_RG_MAXB && Lx >= 2 && Ly >= 2 && (int)P->init_at.size() <= FB_RG_INIT && P->gapless;
    // the longest reach of a site's lists: bwd (the forward sweep's predecessors), fwd without the edges into the end site (the backward sweep's successors)
    std::vector<int> rL, rR, sL, sR;
    if (!both_plain) { rL.assign(Lx + 1, 0); rR.assign(Ly + 1, 0); sL.assign(Lx + 1, 0); sR.assign(Ly + 1, 0); }
    // (two plain sequences: every reach is 1, and nothing below reads the arrays -- such a pair is never a deep-ring pair)
    auto reaches = [&](const pagan_graph *g, const FwdLists &f, int n, std::vector<int> &r, std::vector<int> &s) {
        int longest = 0;
        if (both_plain) return n > 1 ? 1 : 0;
        for (int v = 1; v < n; ++v) {
            for (int k = g->bwd_off[v]; k < g->bwd_off[v + 1]; ++k) r[v] = std::max(r[v], v - g->bwd_src[k]);
            longest = std::max(longest, r[v]);
        }
        for (int v = 0; v < n; ++v)
            for (int k = f.off[v]; k < f.off[v + 1]; ++k) if (f.dst[k] < n) s[v] = std::max(s[v], f.dst[k] - v);
        return longest;
    };
    P->info[0] = nd; P->info[1] = mw;
    P->info[4] = reaches(left, P->fl, Lx, rL, sL); P->info[5] = reaches(right, P->fr, Ly, rR, sR);
    // PAGAN_FB_GROUPS decides alone: that many workgroups a tiled sweep, 1 the one-workgroup kernels, no ring of either kind
    if (sw.groups_set) { P->groups = sw.groups; return; }
    // A long tunnel between plain sequences (every site one edge, from the site before it: leaves) takes the LDS-ring sweeps
    // (pg_fb_forward_ring) ...
    if (sw.ring && nd >= sw.ring_min_nd && shape_ok && both_plain) { P->ring = true; return; }
    // ... and a graph pair (any other edge lists) inside a tunnel the deep-ring sweeps (pg_fb_forward_deep, dp_fb_deep.inc), whose
    // list windows hold FB_DP_E entries of any FB_DP_W consecutive sites
    auto lists_fit = [](const int *off, int n_sites) {
        for (int v = 0; v < n_sites; ++v) if (off[std::min(n_sites, v + FB_DP_W)] - off[v] > FB_DP_E) return false;
        return true;
    };
    if (sw.deep && has_band && nd >= sw.deep_min_nd && shape_ok && !both_plain &&
        lists_fit(left->bwd_off, left->n_sites) && lists_fit(right->bwd_off, right->n_sites) &&
        lists_fit(P->fl.off.data(), left->n_sites) && lists_fit(P->fr.off.data(), right->n_sites)) {
        P->deep = true;
        fb_deep_plan(rL, rR, sL, sR, P);
        return;
    }
    // Wide diagonals: 64 x 64 blocks over as many workgroups as a block anti-diagonal has blocks -- but a pair that is "wide" by a
    // box of its tunnel (one of the 16 leaf pairs has a diagonal of 295 cells) does not need the 64 workgroups of a full matrix at
    // every barrier: a diagonal of mw cells lies in mw / 64 + 2 blocks at most.
    // A long tunnel (round 5; the leaf pairs of 32 x 100 kb: 2e5 diagonals of ~25 cells) on the block schedule as well: its one
    // workgroup paid a __syncthreads() and a round trip to L2 per cell diagonal (2.7 us: 0.55 s a sweep); as blocks it is the few
    // blocks the band has on a block anti-diagonal (fb_live_rows), a wave each, operands in registers / LDS, one counter barrier per
    // 64 diagonals.  Workgroups: the blocks a diagonal of `mw` cells can lie in while it moves through 127 diagonals.
    // PAGAN_FB_BAND_MIN_ND: the shortest pair (in cell diagonals) that takes this path (tests: 0; "off": none).
    const int in_band = (mw + FB_T - 1) / FB_T + 2;
    if (mw > 256) P->groups = std::min({FB_MAX_GROUPS, blocks_x, blocks_y});
    if (P->groups > 1) P->groups = std::max(2, std::min(P->groups, in_band));
    else if (nd >= sw.band_min_nd && Lx >= 2 && Ly >= 2) P->groups = std::max(2, std::min({FB_MAX_GROUPS, in_band, blocks_x, blocks_y}));
}

} // namespace

static int fb_decode_rule(int Lx, int Ly, int widest, bool both_plain, bool gapless, const FbSwitches &sw) {
    return sw.decode_ring && widest <= FB_RG_MAXB && Lx >= 2 && Ly >= 2 && both_plain && gapless ? 1 : 0;
}
int fb_decode_route(const pagan_graph *left, const pagan_graph *right, int Lx, int Ly, const DiagIndex &dx, const FbSwitches &sw) {
    return fb_decode_rule(Lx, Ly, dx.max_width, fb_plain(left) && fb_plain(right), fb_gapless(dx, Lx + Ly - 1), sw);
}

int fb_plan_pair(const pagan_graph *left, const pagan_graph *right, const pagan_band *band, const FbSwitches &sw, FbPlan *P, double l_ng) {
    if (!left || !right || !P) return PAGAN_E_ARG;
    int rc = check_graph(left);
    if (rc == PAGAN_OK) rc = check_graph(right);
    if (rc != PAGAN_OK) return rc;
    *P = FbPlan();
    const int Lx = P->Lx = left->n_sites - 1, Ly = P->Ly = right->n_sites - 1;
    P->nd = Lx + Ly - 1;
    rc = P->rb.build(Lx, Ly, band);
    if (rc != PAGAN_OK) return rc;
    P->dx.build(Lx, Ly, P->rb);
    P->fl = forward_lists(left); P->fr = forward_lists(right);
    fb_corner_init(left, right, l_ng, P);
    P->both_plain = fb_plain(left) && fb_plain(right); P->gapless = fb_gapless(P->dx, P->nd);
    // a thread per cell of the widest diagonal, up to the 1024 of a workgroup (a cell is ~20 exp / log1p calls: a thread with
    // eight cells of a 2,000-cell diagonal was the whole sweep's pace); the deep-ring plan sets its own
    P->block = fb_block_for(P->dx.max_width, true);
    fb_route(left, right, band != nullptr, sw, P);
    if (P->groups > 1) P->block = FB_T;                                       // a wave a block
    if (P->ring) {                                                            // a thread per row of the widest diagonal, or up to three
        P->block = fb_block_for(P->dx.max_width);
        P->nsplit = !sw.ring_split ? 1 : (P->block <= 256 ? 3 : (P->block <= 512 ? 2 : 1));
    }
    P->decode_route = fb_decode_rule(Lx, Ly, P->dx.max_width, P->both_plain, P->gapless, sw);
    P->decode_block = fb_block_for(P->dx.max_width, !P->decode_route);
    return PAGAN_OK;
}

} // namespace fbplan

using namespace fbplan;

extern "C" {

// Host only: what pagan_fb_run would decide for this pair under the current environment (it stages the same plan).
int pagan_fb_debug_route(const pagan_graph *left, const pagan_graph *right, const pagan_band *band, int32_t info[8]) {
    FbPlan plan;
    const int rc = fb_plan_pair(left, right, band, FbSwitches::read(), &plan);
    if (rc != PAGAN_OK) return rc;
    if (info) for (int k = 0; k < 8; ++k) info[k] = plan.info[k];
    return plan.schedule();
}

// Host only: what pagan_fb_decode_batch would decide for this pair under the current environment (it calls the same fb_decode_route).
int pagan_fb_debug_decode_route(const pagan_graph *left, const pagan_graph *right, const pagan_band *band) {
    FbPlan plan;
    const int rc = fb_plan_pair(left, right, band, FbSwitches::read(), &plan);
    return rc != PAGAN_OK ? rc : plan.decode_route;
}

int pagan_fb_debug_plan(const pagan_graph *left, const pagan_graph *right, const pagan_band *band, int32_t n_states, int32_t groups_cap,
                        int32_t groups_cap_b, int32_t head[16], int64_t *init_at, int32_t init_cap, int32_t *seg_start, int32_t *seg_B,
                        int32_t seg_cap, int32_t *dfar, int32_t dfar_cap) {
    if (!head || n_states < 1 || init_cap < 0 || seg_cap < 0 || dfar_cap < 0) return PAGAN_E_ARG;
    FbPlan plan;
    const int rc = fb_plan_pair(left, right, band, FbSwitches::read(), &plan);
    if (rc != PAGAN_OK) return rc;
    const int nseg = (int)plan.seg_B.size();
    const int32_t h[16] = {plan.schedule(), plan.groups, plan.groups_within(groups_cap), plan.groups_within(groups_cap_b), plan.block, plan.nsplit,
                           (int32_t)plan.init_at.size(), plan.init_dmin, nseg, (int32_t)plan.dfar.size(), plan.decode_route, plan.decode_block,
                           fb_table_in_lds(n_states) ? 1 : 0, 0, 0, 0};
    std::memcpy(head, h, sizeof(h));
    auto copy = [](const auto &v, auto *dst, int cap) { for (int k = 0; dst && k < std::min(cap, (int)v.size()); ++k) dst[k] = v[k]; };
    copy(plan.init_at, init_at, init_cap);
    copy(plan.seg_start, seg_start, seg_cap + 1); copy(plan.seg_B, seg_B, seg_cap);
    copy(plan.dfar, dfar, dfar_cap);
    return plan.schedule();
}

// What fb_stage's arena takes: F and B (24 B a cell each), the per-diagonal index and plan (20 B a diagonal), the graphs' lists
// in both directions (sized for four edges a site: 96 B), the score table (up to 211 x 211 doubles) and the record's small
// pieces; then the pool's allowance of a sixteenth (FbArenaPool::take).  Only the lists are an estimate.
int64_t pagan_fb_predict_bytes(int32_t left_sites, int32_t right_sites, const pagan_band *band) {
    const int64_t cells = pagan_dp_count_cells(left_sites, right_sites, band);
    if (cells < 0) return cells;
    const int64_t nd = (int64_t)left_sites + right_sites - 3;
    const int64_t need = 48 * cells + 20 * nd + 96 * ((int64_t)left_sites + right_sites) + (512 << 10) + 8192;
    return need + need / 16;
}

// The constant above was sized for the protein table (211 x 211 logs: 356,168 B of its 532,480); a larger table -- the codon
// model's 1892 x 1892: 28,637,312 B -- comes on top, with the pool's sixteenth.
int64_t pagan_fb_predict_bytes_states(int32_t left_sites, int32_t right_sites, const pagan_band *band, int32_t n_states) {
    if (n_states < 1) return PAGAN_E_ARG;
    const int64_t base = pagan_fb_predict_bytes(left_sites, right_sites, band);
    if (base < 0) return base;
    const int64_t more = std::max<int64_t>(0, 8 * (int64_t)n_states * n_states - 8 * 211 * 211);
    return base + more + more / 16;
}

} // extern "C"
