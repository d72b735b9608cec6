// dp_fb_decode.inc -- included by dp_fb.hip, inside its anonymous namespace, behind dp_fb_sample.inc: posterior decoding.  The one
// alignment a finished pass recommends: the path whose cells carry the largest summed posterior (maximum expected accuracy, as in
// ProbCons / AMAP / FSA), found on the device over the matrices where the sweeps left them.
//
// Cell weight w(s, i, j) = c_s * fb_post(F, B, totals[0]) with c_M = 1 and c_X = c_Y = g (the call's gap weight: 0.5 counts a
// residue once whether it is matched or gapped).  Score matrix A[cell][X, Y, M] in F's layout: A(M, 0, 0) = 0, elsewhere
// A(s, i, j) = w(s, i, j) + max over the cell's predecessors in fs_preds' order -- a match: the k1 x k2 edge pairs, each
// contributing M, X, Y; an X gap: the left edges, each contributing X, Y, M; a Y gap: the right edges, each contributing Y, X, M.
// A candidate counts when the predecessor's A is above -inf AND the transition's own log terms are finite (l_ext; l_open;
// l_ng + l_open; l_ng (+ l_ng) + ltab + edge weights): a transition of probability 0 is no step of any path, whatever the cells
// either side of it hold.  Strict > in list order: the first maximum stays.  A is -inf without a candidate and outside the band,
// so it is finite exactly where F is.  The recurrence is max-plus: nothing transcendental depends on a predecessor (the three
// fb_post of a cell are its own), the file is compiled without contraction.
//
// Three kernels.  pg_fb_decode_fill: any pair, any band -- one workgroup a pair, threads stride over a cell diagonal, a workgroup
// barrier per diagonal (pg_fb_forward's shape).  pg_fb_ring_decode: two plain sequences (fb_decode_route) -- pg_fb_forward_ring's
// shape, one thread a row, the last three diagonals of A in LDS, A to memory unwaited-for, the cell's own F and B requested
// FD_PRE diagonals ahead.  pg_fb_decode_trace: the walk back, one wave a pair and one lane walking; it re-derives every maximum
// from A (same candidates, same rule) and writes the records pagan_internal_replay takes.

#define FD_PRE 4                     // diagonals a ring step's own F / B are requested ahead of their use (divides FB_RG_REFILL)

struct PgFbDecode {
    double g;                        // gap weight
    double *A;                       // [cells][3]
    int *trace;                      // [max_steps][3]
    int *summary;                    // [FB_SUMMARY_INTS]: pg_fb_sample's layout, the objective where that has log_q
    int max_steps;                   // Lx + Ly
    int tab_finite;                  // every entry of the score table has a finite log (then no step looks one up)
};

__device__ __forceinline__ bool fd_fin(double x) { return x > ninf() && x < -ninf(); }

// strict >: the first maximum stays; a transition whose own terms are not finite is no candidate
__device__ __forceinline__ void fd_max(double &best, bool ok, double a) { if (ok && a > best) best = a; }

__global__ __launch_bounds__(1024) void pg_fb_decode_fill(const PgFbJob *jobs, const PgFbDecode *recs) {
    const PgFbJob J = jobs[blockIdx.x];
    const PgFbDecode R = recs[blockIdx.x];
    const double tot = J.totals[0], NI = ninf();
    const bool t_ext = fd_fin(J.l_ext), t_open = fd_fin(J.l_open), t_mo = fd_fin(J.l_ng + J.l_open);
    for (int d = 0; d < J.nd; ++d) {
        const int mn = J.imin[d], mx = J.imax[d];
        const long long off = J.doff[d];
        for (int i = mn + (int)threadIdx.x; i <= mx; i += (int)blockDim.x) {
            const int j = d - i;
            const long long at = off + (i - mn);
            // the cell's own weights first: they do not wait for a predecessor
            const double f0 = J.F[3 * at], f1 = J.F[3 * at + 1], f2 = J.F[3 * at + 2];
            const double b0 = J.B[3 * at], b1 = J.B[3 * at + 1], b2 = J.B[3 * at + 2];
            const double wx = R.g * fb_post(f0, b0, tot), wy = R.g * fb_post(f1, b1, tot), wm = fb_post(f2, b2, tot);
            double ax = NI, ay = NI, am = NI;
            if (i == 0 && j == 0) {
                am = 0.0;
            } else {
                if (i > 0) {
                    double best = NI;
                    for (int k = J.offL[i]; k < J.offL[i + 1]; ++k) {
                        const long long p = cell_at(J, J.srcL[k], j);
                        fd_max(best, t_ext, rd(R.A, p, 0)); fd_max(best, t_open, rd(R.A, p, 1)); fd_max(best, t_mo, rd(R.A, p, 2));
                    }
                    if (best > NI) ax = wx + best;
                }
                if (j > 0) {
                    double best = NI;
                    for (int k = J.offR[j]; k < J.offR[j + 1]; ++k) {
                        const long long p = cell_at(J, i, J.srcR[k]);
                        fd_max(best, t_ext, rd(R.A, p, 1)); fd_max(best, t_open, rd(R.A, p, 0)); fd_max(best, t_mo, rd(R.A, p, 2));
                    }
                    if (best > NI) ay = wy + best;
                }
                if (i > 0 && j > 0) {
                    const double sc = J.ltab[J.stL[i] + (long long)J.stR[j] * J.S];
                    double best = NI;
                    for (int k1 = J.offL[i]; k1 < J.offL[i + 1]; ++k1)
                        for (int k2 = J.offR[j]; k2 < J.offR[j + 1]; ++k2) {
                            const long long p = cell_at(J, J.srcL[k1], J.srcR[k2]);
                            const double w = (double)J.lwL[k1] + (double)J.lwR[k2];
                            const bool t_mm = fd_fin(J.l_ng + J.l_ng + sc + w), t_xm = fd_fin(J.l_ng + sc + w);
                            fd_max(best, t_mm, rd(R.A, p, 2)); fd_max(best, t_xm, rd(R.A, p, 0)); fd_max(best, t_xm, rd(R.A, p, 1));
                        }
                    if (best > NI) am = wm + best;
                }
            }
            double *o = R.A + 3 * at;
            o[0] = ax; o[1] = ay; o[2] = am;
        }
        __syncthreads();
    }
}

// ---- two plain sequences: one workgroup, thread x owns row x mod B, the last three diagonals of A in an LDS ring ----
// (pg_fb_ring_decode, not pg_fb_decode_ring: test_fb_asm_cpu.py counts every kernel named pg_fb_*_ring as one of the sixteen sweeps.)
// pg_fb_forward_ring's step with max in the place of log-sum-exp, one thread a row (there are no sums to split over states).  What
// the sweep does not have: the cell's own F and B come from memory.  A wave's loads and stores retire in order behind one
// counter, so a load requested on the step it is used would wait for the step before's stores of A; the six values of a row are
// requested FD_PRE diagonals ahead instead, rotated through registers (the loop is unrolled FD_PRE times, a slot per step of the
// unrolled body), and the step's wait is a counted one that leaves everything requested since outstanding.  The loads are issued
// unconditionally (an idle thread reads cell 0): no branch lies between a request and its use that holds a memory operation on
// one side only, which is what lets the compiler count.  The diagonals' windows hold FD_PRE entries more than a refill's span.
#define FD_WIN (2 * FB_RG_REFILL)    // entries of the diagonals' windows (>= FB_RG_REFILL + FD_PRE)
template <int MAXB>
struct FdRingSmem {
    static constexpr int COLS = MAXB > 512 ? 2048 : FB_RG_COLS;
    double ring[3][3][MAXB];             // [diagonal slot][X, Y, M][thread]
    int c_st[COLS]; float c_lw[COLS];    // column j at j % COLS: state, log weight of the edge (j-1) -> j
    int r_st[COLS]; float r_lw[COLS];
    int dmin[FD_WIN], dmax[FD_WIN]; long long doff[FD_WIN];   // diagonal d at d % FD_WIN
    double ltab[256];
};

// TAB: the launch holds a pair whose score table has an entry of probability 0, and a match step looks its entry up (from LDS, or
// from memory when the table does not fit: that load waits for the step before's stores).  Without it -- every model the project
// builds -- the lookup is not compiled at all: behind a branch that may have issued a load the compiler waits for everything.
template <int MAXB, bool TAB>
__global__ __launch_bounds__(FB_RG_THREADS) void pg_fb_ring_decode(const PgFbJob *jobs, const PgFbDecode *recs) {
    __shared__ FdRingSmem<MAXB> M;
    constexpr int CMASK = FdRingSmem<MAXB>::COLS - 1;
    const PgFbJob J = jobs[blockIdx.x];
    const PgFbDecode R = recs[blockIdx.x];
    const int tid = (int)threadIdx.x, nt = (int)blockDim.x, B = nt, x = tid;
    const int xm1 = (x - 1) & (B - 1);
    const double NI = ninf(), tot = J.totals[0], g = R.g;
    const bool tab_lds = J.S * J.S <= 256;
    const bool t_ext = fd_fin(J.l_ext), t_open = fd_fin(J.l_open), t_mo = fd_fin(J.l_ng + J.l_open);
    if (TAB && tab_lds) for (int k = tid; k < J.S * J.S; k += nt) M.ltab[k] = J.ltab[k];
    for (int q = 0; q < 9; ++q) (&M.ring[0][0][0])[q * MAXB + x] = NI;
    int mn1 = 0, mx1 = -1, mn2 = 0, mx2 = -1;            // the intervals of the diagonals d-1, d-2
    int s0 = 0, s1 = 2, s2 = 1;                          // ring slots of d, d-1, d-2
    int cols_hi = -1, rows_hi = -1;
    const fb_gcd F = (fb_gcd)(unsigned long long)J.F, Bw = (fb_gcd)(unsigned long long)J.B;
    const fb_gd A = (fb_gd)(unsigned long long)R.A;
    // the windows of the diagonals [d, d + FB_RG_REFILL + FD_PRE), their rows and columns
    auto refill = [&](int d) {
        for (int k = tid; k < FB_RG_REFILL + FD_PRE; k += nt) {
            const int dd = d + k;
            const bool in = dd < J.nd;
            M.dmin[dd & (FD_WIN - 1)] = in ? J.imin[dd] : 0; M.dmax[dd & (FD_WIN - 1)] = in ? J.imax[dd] : -1;
            M.doff[dd & (FD_WIN - 1)] = in ? J.doff[dd] : 0;
        }
        const int mn_ = J.imin[d], mx_ = J.imax[d];
        const int want_c = min(J.Ly - 1, d - mn_ + FB_RG_REFILL), want_r = min(J.Lx - 1, mx_ + FB_RG_REFILL);
        for (int j = cols_hi + 1 + tid; j <= want_c; j += nt) {
            M.c_st[j & CMASK] = J.stR[j];
            M.c_lw[j & CMASK] = j > 0 ? J.lwR[j - 1] : 0.0f;       // (plain graph: site j's one edge is list entry j - 1)
        }
        for (int i = rows_hi + 1 + tid; i <= want_r; i += nt) {
            M.r_st[i & CMASK] = J.stL[i];
            M.r_lw[i & CMASK] = i > 0 ? J.lwL[i - 1] : 0.0f;
        }
        cols_hi = max(cols_hi, want_c); rows_hi = max(rows_hi, want_r);
        fb_lds_barrier();
    };
    // the thread's cell on diagonal dd (cell 0 where it has none: the load is issued all the same)
    auto own_cell = [&](int dd) -> long long {
        const int w = dd & (FD_WIN - 1);
        const int mn = M.dmin[w], mx = M.dmax[w];
        const int i = mn + ((x - mn) & (B - 1));
        return i <= mx ? M.doff[w] + (i - mn) : 0;
    };
    double pf[FD_PRE][6];
    __syncthreads();
    refill(0);
#pragma unroll
    for (int u = 0; u < FD_PRE; ++u) {
        const long long at = own_cell(u);
        pf[u][0] = F[3 * at]; pf[u][1] = F[3 * at + 1]; pf[u][2] = F[3 * at + 2];
        pf[u][3] = Bw[3 * at]; pf[u][4] = Bw[3 * at + 1]; pf[u][5] = Bw[3 * at + 2];
    }
    // (steps beyond the last diagonal, up to a multiple of FD_PRE: every thread idle)
    for (int d0 = 0; d0 < J.nd; d0 += FD_PRE) {
        if (d0 > 0 && (d0 & (FB_RG_REFILL - 1)) == 0) refill(d0);
#pragma unroll
        for (int u = 0; u < FD_PRE; ++u) {
            const int d = d0 + u;
            const int mn = M.dmin[d & (FD_WIN - 1)], mx = M.dmax[d & (FD_WIN - 1)];
            const int i = mn + ((x - mn) & (B - 1));
            const bool active = i <= mx;
            // the weights first, by every thread, and only then the request for the row's cell FD_PRE diagonals on: the six
            // values are dead by then and the request lands in their registers (requested before, it took registers of its own and
            // the loop's end moved them into place -- a move waits for the load it moves)
            const double wx = g * fb_post(pf[u][0], pf[u][3], tot), wy = g * fb_post(pf[u][1], pf[u][4], tot), wm = fb_post(pf[u][2], pf[u][5], tot);
            __builtin_amdgcn_sched_barrier(0);
            {
                const long long at = own_cell(d + FD_PRE);
                pf[u][0] = F[3 * at]; pf[u][1] = F[3 * at + 1]; pf[u][2] = F[3 * at + 2];
                pf[u][3] = Bw[3 * at]; pf[u][4] = Bw[3 * at + 1]; pf[u][5] = Bw[3 * at + 2];
            }
            __builtin_amdgcn_sched_barrier(0);
            double ax = NI, ay = NI, am = NI;
            if (active) {
                const int j = d - i;
                if (i == 0 && j == 0) {
                    am = 0.0;
                } else {
                    if (i > 0 && i - 1 >= mn1 && i - 1 <= mx1) {                   // (i-1, j): X, Y, M
                        double best = NI;
                        fd_max(best, t_ext, M.ring[s1][0][xm1]); fd_max(best, t_open, M.ring[s1][1][xm1]); fd_max(best, t_mo, M.ring[s1][2][xm1]);
                        if (best > NI) ax = wx + best;
                    }
                    if (j > 0 && i >= mn1 && i <= mx1) {                           // (i, j-1): Y, X, M
                        double best = NI;
                        fd_max(best, t_ext, M.ring[s1][1][x]); fd_max(best, t_open, M.ring[s1][0][x]); fd_max(best, t_mo, M.ring[s1][2][x]);
                        if (best > NI) ay = wy + best;
                    }
                    if (i > 0 && j > 0 && i - 1 >= mn2 && i - 1 <= mx2) {          // (i-1, j-1): M, X, Y
                        const double w = (double)M.r_lw[i & CMASK] + (double)M.c_lw[j & CMASK];
                        double sc = 0.0;
                        if (TAB) sc = fb_score<false>(tab_lds, M.ltab, J.ltab, M.r_st[i & CMASK], M.c_st[j & CMASK], J.S);
                        const bool t_mm = fd_fin(J.l_ng + J.l_ng + sc + w), t_xm = fd_fin(J.l_ng + sc + w);
                        double best = NI;
                        fd_max(best, t_mm, M.ring[s2][2][xm1]); fd_max(best, t_xm, M.ring[s2][0][xm1]); fd_max(best, t_xm, M.ring[s2][1][xm1]);
                        if (best > NI) am = wm + best;
                    }
                }
                const fb_gd o = A + 3 * (M.doff[d & (FD_WIN - 1)] + (i - mn));
                o[0] = ax; o[1] = ay; o[2] = am;
            }
            M.ring[s0][0][x] = ax; M.ring[s0][1][x] = ay; M.ring[s0][2][x] = am;
            mn2 = mn1; mx2 = mx1; mn1 = mn; mx1 = mx;
            { const int t = s2; s2 = s1; s1 = s0; s0 = t; }
            fb_lds_barrier();
        }
    }
}

// ---- the walk back ----
// One wave a pair (a level's walks overlap), lane 0 walking: a step is a chain of dependent loads with nothing beside it.  The
// pair's record sits in LDS as in pg_fb_sample (as uniform values its pointers took more scalar registers than a wave has).
// V.F points at A: FsJob::cell gives the three A of a cell, -inf outside the band.  No exp, no mix, no F.

// the end corner's candidates in fs_corner's order: fn(a, state, i, j, k1, k2); a = -inf where the transition is none
template <class Fn>
__device__ __forceinline__ void fd_corner(const FsJob &J, Fn &&fn) {
    const int l0 = J.offL[J.Lx], l1 = J.offL[J.Lx + 1], r0 = J.offR[J.Ly], r1 = J.offR[J.Ly + 1];
    if (!(l1 > l0 && r1 > r0)) return;
    auto mt = [&](int k1, int k2) {
        const int p = J.srcL[k1], q = J.srcR[k2];
        double a0, a1, a2;
        J.cell(p, q, a0, a1, a2);
        fn(fd_fin(J.ng + (double)J.lwL[k1] + (double)J.lwR[k2]) ? a2 : ninf(), 2, p, q, k1 - l0, k2 - r0);
    };
    auto xc = [&](int k1) {
        const int p = J.srcL[k1];
        double a0, a1, a2;
        J.cell(p, J.Ly - 1, a0, a1, a2);
        fn(a0, 0, p, J.Ly - 1, k1 - l0, -1);
    };
    auto yc = [&](int k2) {
        const int q = J.srcR[k2];
        double a0, a1, a2;
        J.cell(J.Lx - 1, q, a0, a1, a2);
        fn(a1, 1, J.Lx - 1, q, -1, k2 - r0);
    };
    for (int k1 = l0; k1 < l1; ++k1)
        for (int k2 = r0; k2 < r1; ++k2) {
            mt(k1, k2);
            if (k2 == r0) xc(k1);
            if (k2 > r0 || k1 == l0) yc(k2);
        }
}

// the candidates of cell (i, j) in `state`, in fs_preds' order: fn(a, state, p, q, k1, k2)
template <class Fn>
__device__ __forceinline__ void fd_preds(const FsJob &J, int state, int i, int j, Fn &&fn) {
    const bool mvL = state != PAGAN_Y_MAT, mvR = state != PAGAN_X_MAT;
    const int a0 = mvL ? J.offL[i] : 0, a1 = mvL ? J.offL[i + 1] : 1;
    const int b0 = mvR ? J.offR[j] : 0, b1 = mvR ? J.offR[j + 1] : 1;
    const double NI = ninf();
    double sc = 0.0;
    if (state == PAGAN_M_MAT) sc = J.ltab[J.stL[i] + (long long)J.stR[j] * J.S];
    const bool t_ext = fd_fin(J.ext), t_open = fd_fin(J.open), t_mo = fd_fin(J.ng + J.open);
    for (int k1 = a0; k1 < a1; ++k1) {
        const int p = mvL ? J.srcL[k1] : i;
        const double wl = mvL ? (double)J.lwL[k1] : 0.0;
        for (int k2 = b0; k2 < b1; ++k2) {
            const int q = mvR ? J.srcR[k2] : j;
            double c0, c1, c2;
            J.cell(p, q, c0, c1, c2);
            const int ka = mvL ? k1 - a0 : 0, kb = mvR ? k2 - b0 : 0;
            if (state == PAGAN_M_MAT) {
                const double w = wl + (double)J.lwR[k2];
                const bool t_mm = fd_fin(J.ng + J.ng + sc + w), t_xm = fd_fin(J.ng + sc + w);
                fn(t_mm ? c2 : NI, 2, p, q, ka, kb); fn(t_xm ? c0 : NI, 0, p, q, ka, kb); fn(t_xm ? c1 : NI, 1, p, q, ka, kb);
            } else if (state == PAGAN_X_MAT) {
                fn(t_ext ? c0 : NI, 0, p, q, ka, kb); fn(t_open ? c1 : NI, 1, p, q, ka, kb); fn(t_mo ? c2 : NI, 2, p, q, ka, kb);
            } else {
                fn(t_ext ? c1 : NI, 1, p, q, ka, kb); fn(t_open ? c0 : NI, 0, p, q, ka, kb); fn(t_mo ? c2 : NI, 2, p, q, ka, kb);
            }
        }
    }
}

__global__ __launch_bounds__(64) void pg_fb_decode_trace(const PgFbJob *jobs, const PgFbDecode *recs) {
    __shared__ FsJob J;
    __shared__ PgFbDecode R;
    if (threadIdx.x == 0) {
        J = fs_job_of(jobs[blockIdx.x]); R = recs[blockIdx.x];
        J.F = (fb_gcd)(unsigned long long)R.A;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    const fs_go trace = (fs_go)(unsigned long long)R.trace, out = (fs_go)(unsigned long long)R.summary;
    const double NI = ninf();
    int status = 0, steps = 0, n_m = 0, n_x = 0, n_y = 0;
    int state = 0, i = 0, j = 0, e_k1 = -1, e_k2 = -1;
    double objective = 0.0;
    {
        double best = NI;
        fd_corner(J, [&](double a, int s, int p, int q, int ka, int kb) {
            if (a > best) { best = a; state = s; i = p; j = q; e_k1 = ka; e_k2 = kb; }
        });
        if (best > NI) objective = best; else status = 1;             // no end candidate: the full probability is 0
    }
    const int e_state = state, e_i = i, e_j = j;
    while (status == 0 && !(i < 1 && j < 1)) {
        double best = NI;
        int ps = 0, pi = 0, pj = 0, pk1 = 0, pk2 = 0;
        fd_preds(J, state, i, j, [&](double a, int s, int p, int q, int ka, int kb) {
            if (a > best) { best = a; ps = s; pi = p; pj = q; pk1 = ka; pk2 = kb; }
        });
        if (!(best > NI) || steps >= R.max_steps) { status = 2; break; }
        const fs_go t = trace + 3ll * steps;
        t[0] = i; t[1] = j; t[2] = (int)((unsigned)state | ((unsigned)pk1 << 4) | ((unsigned)pk2 << 18));
        ++steps;
        n_m += state == PAGAN_M_MAT; n_x += state == PAGAN_X_MAT; n_y += state == PAGAN_Y_MAT;
        state = ps; i = pi; j = pj;
    }
    out[FB_SUM_STATUS] = status;
    out[FB_SUM_END] = e_state; out[FB_SUM_END + 1] = e_i; out[FB_SUM_END + 2] = e_j; out[FB_SUM_END + 3] = e_k1; out[FB_SUM_END + 4] = e_k2;
    out[FB_SUM_STEPS] = steps; out[FB_SUM_M] = n_m; out[FB_SUM_X] = n_x; out[FB_SUM_Y] = n_y;
    const long long ob = __double_as_longlong(objective);
    out[FB_SUM_VALUE] = (int)(unsigned)(ob & 0xffffffffll); out[FB_SUM_VALUE + 1] = (int)(unsigned)((unsigned long long)ob >> 32);
    out[12] = out[13] = out[14] = out[15] = 0;
}
