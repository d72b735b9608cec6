// dp_fb_deep.inc -- included by dp_fb.hip: the LDS-ring sweeps for GRAPH pairs inside a tunnel (pg_fb_forward_deep /
// pg_fb_backward_deep).  The host's side -- who takes them (fb_route) and the plan (fb_deep_plan) -- is in dp_fb_plan.cpp.
//
// Same frame as the ring sweeps of plain sequences (dp_fb.hip, pg_fb_forward_ring): one workgroup a pair, thread x owns the row
// i = x (mod B) of the current diagonal, a step ends in s_waitcnt lgkmcnt(0) + s_barrier, the scores leave for memory
// unwaited-for.  What a graph pair changes:
//  * a site has a LIST of edges and an edge may jump over skipped sites: a left edge of reach r = i - src puts the X predecessor
//    r diagonals back, a right edge of reach s the Y predecessor s back, a match through both r + s back.  The ring holds the last
//    D diagonals, ring[D][3][B] doubles with D * B = FB_DP_CELLS (96 KB), and a slot is valid if the row was in the band on that
//    diagonal (two compares against its interval; the intervals' window keeps the last 256 diagonals across a refill).
//  * the host cuts the pair's diagonals into SEGMENTS, each with the smallest B in {64 .. 1,024} that holds its widest diagonal
//    (and the 64 diagonals either side of it, so that the ring can be rebuilt in the segment's layout) and D = FB_DP_CELLS / B; at
//    a boundary every wave drains its stores, the workgroup meets, and the last D - 1 diagonals are read back from the stored
//    matrix (loads that go to the L2) into the ring in the new layout.  B, D and the thread-per-state split are run-time values.
//  * the rows' and the columns' windows hold each site's state and its list (offset; per entry the other end and the log weight),
//    restaged from their first row / column every FB_DP_REFILL diagonals.
//  * FAR edges: a predecessor further back than D - 1 diagonals has left the ring and is read from the stored matrix.  Safe
//    because (a) in a segment that holds such a cell every wave drains its stores (s_waitcnt vmcnt(0)) before the step barrier of
//    every (D/2)-th diagonal, so a store of diagonal d' is complete, for every wave of the workgroup, behind the barrier of a step
//    <= d' + D/2 - 1 < d' + D, and a segment boundary drains everything; (b) the load is an agent-scope load (sc1: it is served
//    by the L2, which the workgroup's write-through stores have reached, never by a stale line of the compute unit's L1).  The
//    host marks the diagonals that hold a far cell (pagan_fb_debug_route counts them); a diagonal without one takes a step that
//    holds no load from memory and no vmcnt wait.

#define FB_DP_REFILL 256

typedef const __attribute__((address_space(1))) unsigned long long *fb_gcu;

// a score read from the stored matrix: agent scope (global_load ... sc1), see above
__device__ __forceinline__ double fb_far_ld(const double *p) {
    return __longlong_as_double((long long)__hip_atomic_load((fb_gcu)(unsigned long long)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
}
__device__ __forceinline__ double fb_far_rd(const PgFbJob &J, const double *A, int p, int q, int s) {
    const long long at = cell_at(J, p, q);
    return at >= 0 ? fb_far_ld(A + 3 * at + s) : ninf();
}
// The far path's loads, issued as inline asm with their own wait (as dp_kcommon.h's far_cell): the compiler's waitcnt insertion never
// sees a load in flight, so it places no vmcnt(0) -- which would also wait for every store in flight -- on a step without far cells.
__device__ __forceinline__ double fb_far_f64(const double *p) {
    double v;
    asm volatile("global_load_dwordx2 %0, %1, off sc1\n\ts_waitcnt vmcnt(0)" : "=&v"(v) : "v"((fb_gcd)(unsigned long long)p) : "memory");
    return v;
}
__device__ __forceinline__ void fb_far_cell(const double *p, double &xs, double &ys, double &ms) {
    typedef double fb_d2 __attribute__((ext_vector_type(2)));
    fb_d2 xy; double m;
    asm volatile("global_load_dwordx4 %0, %2, off sc1\n\tglobal_load_dwordx2 %1, %2, off offset:16 sc1\n\ts_waitcnt vmcnt(0)"
                 : "=&v"(xy), "=&v"(m) : "v"((fb_gcd)(unsigned long long)p) : "memory");
    xs = xy.x; ys = xy.y; ms = m;
}
// (read-only inputs: no cache policy needed)
__device__ __forceinline__ int fb_far_i32(const int *p) {
    int v;
    asm volatile("global_load_dword %0, %1, off\n\ts_waitcnt vmcnt(0)" : "=&v"(v) : "v"((const __attribute__((address_space(1))) int *)(unsigned long long)p) : "memory");
    return v;
}
__device__ __forceinline__ long long fb_far_i64(const long long *p) {
    long long v;
    asm volatile("global_load_dwordx2 %0, %1, off\n\ts_waitcnt vmcnt(0)" : "=&v"(v) : "v"((const __attribute__((address_space(1))) long long *)(unsigned long long)p) : "memory");
    return v;
}
// a = log(exp(a) + exp(v)); lse(-inf, v) is v to the bit (1 + e^-60 rounds to 1), so the first term of a sum costs nothing
__device__ __forceinline__ void fb_acc(double &a, double v) {
    if (a == ninf()) a = v; else a = lse(a, v);
}

struct FbDeepSmem {
    double ring[3 * FB_DP_CELLS];                        // [(d % D) * 3 + state][row % B]
    int r_st[FB_DP_W], r_off[FB_DP_W + 8];               // row rbase + k: state, first list entry (relative to the window's first)
    int c_st[FB_DP_W], c_off[FB_DP_W + 8];
    int r_e[FB_DP_E], c_e[FB_DP_E];                      // list entries: the edge's other end (forward: source, backward: destination)
    float r_lw[FB_DP_E], c_lw[FB_DP_E];
    int dmin[2 * FB_DP_REFILL], dmax[2 * FB_DP_REFILL];  // diagonal d at d % 512: a refill leaves the 256 before (forward) / after (backward) readable
    long long doff[FB_DP_REFILL]; int dfar[FB_DP_REFILL];
    double ltab[256];
    long long i_at[FB_RG_INIT]; double i_val[FB_RG_INIT];
};

// Who a thread is in a segment of B rows: three threads a row up to B = 256 (one per state), two with 512 (X and Y; M), one with
// 1,024; threads beyond are idle until a segment needs them (the workgroup has min(1,024, 3 * widest B) threads).
#define FB_DEEP_WHO                                                                                           \
    const int nsplit = B <= 256 ? 3 : (B <= 512 ? 2 : 1);                                                     \
    const int part = (tid >> 6) % nsplit;                                                                     \
    x = ((tid >> 6) / nsplit) * 64 + (tid & 63);                                                              \
    live = x < B;                                                                                             \
    do_x = nsplit == 1 || part == 0; do_y = nsplit == 1 || (nsplit == 2 ? part == 0 : part == 1); do_m = nsplit == 1 || part == nsplit - 1;

// the three scores of (row p, diagonal dd), `reach` diagonals from the current one: from the ring, or (FAR) from memory
template <bool FAR>
__device__ __forceinline__ void fb_deep_cell3(const FbDeepSmem &M, const PgFbJob &J, const double *A, int B, int D, int dd, int reach, int p,
                                              double &vx, double &vy, double &vm) {
    vx = ninf(); vy = ninf(); vm = ninf();
    if (!FAR || reach < D) {
        if (p >= M.dmin[dd & (2 * FB_DP_REFILL - 1)] && p <= M.dmax[dd & (2 * FB_DP_REFILL - 1)]) {
            const double *r = &M.ring[(dd & (D - 1)) * 3 * B + (p & (B - 1))];
            vx = r[0]; vy = r[B]; vm = r[2 * B];
        }
    } else {
        const int lo = fb_far_i32(J.imin + dd), hi = fb_far_i32(J.imax + dd);
        if (p >= lo && p <= hi) fb_far_cell(A + 3 * (fb_far_i64(J.doff + dd) + (p - lo)), vx, vy, vm);
    }
}
template <bool FAR>
__device__ __forceinline__ double fb_deep_cell1(const FbDeepSmem &M, const PgFbJob &J, const double *A, int B, int D, int dd, int reach, int p, int s) {
    if (!FAR || reach < D) {
        if (p >= M.dmin[dd & (2 * FB_DP_REFILL - 1)] && p <= M.dmax[dd & (2 * FB_DP_REFILL - 1)])
            return M.ring[((dd & (D - 1)) * 3 + s) * B + (p & (B - 1))];
        return ninf();
    }
    const int lo = fb_far_i32(J.imin + dd), hi = fb_far_i32(J.imax + dd);
    double v = ninf();
    if (p >= lo && p <= hi) v = fb_far_f64(A + 3 * (fb_far_i64(J.doff + dd) + (p - lo)) + s);
    return v;
}

// one cell of the forward sweep, the states this thread owns (the recurrence of pg_fb_forward)
template <bool ALL_LDS, bool FAR>
__device__ __forceinline__ void fb_deep_fwd_cell(const FbDeepSmem &M, const PgFbJob &J, bool tab_lds, int B, int D, int d, int i, int rbase, int cbase,
                                                 bool do_x, bool do_y, bool do_m, double &fx, double &fy, double &fm) {
    const int j = d - i;
    if (i == 0 && j == 0) { fm = 0.0; return; }                                    // fwd_score = 1, VA:730
    const int ri = i - rbase, cj = j - cbase;
    const int l0 = M.r_off[ri], l1 = i > 0 ? M.r_off[ri + 1] : l0, q0 = M.c_off[cj], q1 = j > 0 ? M.c_off[cj + 1] : q0;
    if (do_x)
        for (int k = l0; k < l1; ++k) {                                             // VA:2153, 2184, 2215
            const int p = M.r_e[k], r = i - p;
            double ax, ay, am;
            fb_deep_cell3<FAR>(M, J, J.F, B, D, d - r, r, p, ax, ay, am);
            fb_acc(fx, lse3(ax + J.l_ext, ay + J.l_open, am + J.l_ng + J.l_open));
        }
    if (do_y)
        for (int k = q0; k < q1; ++k) {
            const int s = j - M.c_e[k];
            double px, py, pm;
            fb_deep_cell3<FAR>(M, J, J.F, B, D, d - s, s, i, px, py, pm);
            fb_acc(fy, lse3(py + J.l_ext, px + J.l_open, pm + J.l_ng + J.l_open));
        }
    if (do_m && l1 > l0 && q1 > q0) {
        const double sc = fb_score<ALL_LDS>(tab_lds, M.ltab, J.ltab, M.r_st[ri], M.c_st[cj], J.S);
        const double mm = J.l_ng + J.l_ng + sc, xm = J.l_ng + sc;                  // VA:1383-1391
        for (int k1 = l0; k1 < l1; ++k1)
            for (int k2 = q0; k2 < q1; ++k2) {                                      // VA:2051, 2080, 2108
                const int p = M.r_e[k1], rs = (i - p) + (j - M.c_e[k2]);
                const double w = (double)M.r_lw[k1] + (double)M.c_lw[k2];
                double cx, cy, cm;
                fb_deep_cell3<FAR>(M, J, J.F, B, D, d - rs, rs, p, cx, cy, cm);
                fb_acc(fm, lse3(cm + mm + w, cx + xm + w, cy + xm + w));
            }
    }
}

template <bool ALL_LDS>
__global__ __launch_bounds__(FB_RG_THREADS) void pg_fb_forward_deep(const PgFbJob *jobs) {
    __shared__ FbDeepSmem M;
    const PgFbJob J = jobs[blockIdx.x];
    const int tid = (int)threadIdx.x, nt = (int)blockDim.x;
    const double NI = ninf();
    const bool tab_lds = J.S * J.S <= 256;
    if (tab_lds) for (int k = tid; k < J.S * J.S; k += nt) M.ltab[k] = J.ltab[k];
    const fb_gd F = (fb_gd)(unsigned long long)J.F;
    int seg = -1, seg_end = 0, B = 64, D = FB_DP_CELLS / 64, x = 0, drain = 0;
    bool live = false, do_x = false, do_y = false, do_m = false;
    int rbase = 0, cbase = 0;
    __syncthreads();
    for (int d = 0; d < J.nd; ++d) {
        if (d == seg_end) {
            // the next segment: its B, D, who the thread is; the ring of the last D - 1 diagonals in the new layout
            ++seg;
            const int sb = J.seg_B[seg];
            B = sb & 0xffff; D = FB_DP_CELLS / B; drain = (sb >> 16) ? (D / 2 - 1) : -1;
            seg_end = J.seg_start[seg + 1];
            FB_DEEP_WHO
            if (d > 0) {
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __syncthreads();
                for (int dd = max(0, d - (D - 1)); dd < d; ++dd) {
                    const int lo = J.imin[dd], n3 = 3 * (J.imax[dd] - lo + 1);
                    const double *src = J.F + 3 * J.doff[dd];
                    for (int k = tid; k < n3; k += nt) M.ring[((dd & (D - 1)) * 3 + k % 3) * B + ((lo + k / 3) & (B - 1))] = fb_far_ld(src + k);
                }
                __syncthreads();
            }
        }
        if ((d & (FB_DP_REFILL - 1)) == 0) {
            // the next FB_DP_REFILL diagonals, their rows and columns (the largest of either grows by at most one a diagonal) with their lists
            for (int k = tid; k < FB_DP_REFILL; k += nt) {
                const int dd = d + k;
                const bool in = dd < J.nd;
                M.dmin[dd & (2 * FB_DP_REFILL - 1)] = in ? J.imin[dd] : 0; M.dmax[dd & (2 * FB_DP_REFILL - 1)] = in ? J.imax[dd] : -1;
                M.doff[k] = in ? J.doff[dd] : 0; M.dfar[k] = in ? J.dfar[dd] : 0;
            }
            const int mn_ = J.imin[d], mx_ = J.imax[d];
            rbase = mn_; cbase = d - mx_;
            const int n_r = min(min(J.Lx - rbase, mx_ - mn_ + 1 + FB_DP_REFILL), FB_DP_W), n_c = min(min(J.Ly - cbase, mx_ - mn_ + 1 + FB_DP_REFILL), FB_DP_W);
            const int e_r = J.offL[rbase], e_c = J.offR[cbase];
            const int n_er = min(J.offL[rbase + n_r] - e_r, FB_DP_E), n_ec = min(J.offR[cbase + n_c] - e_c, FB_DP_E);
            for (int k = tid; k <= n_r; k += nt) { M.r_off[k] = J.offL[rbase + k] - e_r; if (k < n_r) M.r_st[k] = J.stL[rbase + k]; }
            for (int k = tid; k <= n_c; k += nt) { M.c_off[k] = J.offR[cbase + k] - e_c; if (k < n_c) M.c_st[k] = J.stR[cbase + k]; }
            for (int k = tid; k < n_er; k += nt) { M.r_e[k] = J.srcL[e_r + k]; M.r_lw[k] = J.lwL[e_r + k]; }
            for (int k = tid; k < n_ec; k += nt) { M.c_e[k] = J.srcR[e_c + k]; M.c_lw[k] = J.lwR[e_c + k]; }
            fb_lds_barrier();                                      // (the staged values went through registers into LDS: the loads are done)
        }
        const int mn = M.dmin[d & (2 * FB_DP_REFILL - 1)], mx = M.dmax[d & (2 * FB_DP_REFILL - 1)];
        const int i = mn + ((x - mn) & (B - 1));
        if (live && i <= mx) {
            double fx = NI, fy = NI, fm = NI;
            if (M.dfar[d & (FB_DP_REFILL - 1)] & 1) {
                fb_deep_fwd_cell<ALL_LDS, true>(M, J, tab_lds, B, D, d, i, rbase, cbase, do_x, do_y, do_m, fx, fy, fm);
            } else {
                asm volatile("s_nop 13" ::: "memory");             // (tests/test_fb_deep_cpu.py: the step of a diagonal without a far cell lies between these two)
                fb_deep_fwd_cell<ALL_LDS, false>(M, J, tab_lds, B, D, d, i, rbase, cbase, do_x, do_y, do_m, fx, fy, fm);
                asm volatile("s_nop 14" ::: "memory");
            }
            const fb_gd o = F + 3 * (M.doff[d & (FB_DP_REFILL - 1)] + (i - mn));
            double *r = &M.ring[(d & (D - 1)) * 3 * B + x];
            if (do_x) { o[0] = fx; r[0] = fx; }
            if (do_y) { o[1] = fy; r[B] = fy; }
            if (do_m) { o[2] = fm; r[2 * B] = fm; }
        }
        if (drain >= 0 && (d & drain) == 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // far reads: stores older than D diagonals are complete
        fb_lds_barrier();
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();                                                               // (the end corner reads the scores from memory)
    if (threadIdx.x == 0)
        J.totals[0] = fb_end_corner(J, [&](int p, int q, int s_) { return fb_far_rd(J, J.F, p, q, s_); });
}

// one cell of the backward sweep (the recurrence of pg_fb_backward: the sums are taken one by one, in its order); the windows
// hold the FORWARD lists (destination, log weight) and the states of the rows / columns a near edge reaches
template <bool ALL_LDS, bool FAR>
__device__ __forceinline__ void fb_deep_bwd_cell(const FbDeepSmem &M, const PgFbJob &J, bool tab_lds, int B, int D, int d, int i, int rbase, int cbase,
                                                 int n_r, int n_c, bool do_x, bool do_y, bool do_m, double &bx, double &by, double &bm) {
    const int j = d - i;
    const int ri = i - rbase, cj = j - cbase;
    const int l0 = M.r_off[ri], l1 = M.r_off[ri + 1], q0 = M.c_off[cj], q1 = M.c_off[cj + 1];
    for (int k = l0; k < l1; ++k) {                                                 // iterate_fwd_edges_for_gap, left site
        const int t = M.r_e[k];
        if (t >= J.Lx) continue;                                                    // VA:1580
        const double nx = fb_deep_cell1<FAR>(M, J, J.B, B, D, d + (t - i), t - i, t, 0);
        if (do_x) fb_acc(bx, nx + J.l_ext);                                         // VA:2281-2303
        if (do_y) fb_acc(by, nx + J.l_open);
        if (do_m) fb_acc(bm, nx + J.l_ng + J.l_open);
    }
    for (int k = q0; k < q1; ++k) {
        const int u = M.c_e[k];
        if (u >= J.Ly) continue;
        const double ny = fb_deep_cell1<FAR>(M, J, J.B, B, D, d + (u - j), u - j, i, 1);
        if (do_y) fb_acc(by, ny + J.l_ext);
        if (do_x) fb_acc(bx, ny + J.l_open);
        if (do_m) fb_acc(bm, ny + J.l_ng + J.l_open);
    }
    for (int k1 = l0; k1 < l1; ++k1)                                                // iterate_fwd_edges_for_match
        for (int k2 = q0; k2 < q1; ++k2) {
            const int t = M.r_e[k1], u = M.c_e[k2];
            if (t >= J.Lx || u >= J.Ly) continue;
            const int rs = (t - i) + (u - j);
            // (a near edge's other end is in the windows: they reach FB_DP_HALO sites past the diagonal's last row / column)
            int stt, stu;
            if (!FAR || t - rbase < n_r) stt = M.r_st[t - rbase]; else stt = fb_far_i32(J.stL + t);
            if (!FAR || u - cbase < n_c) stu = M.c_st[u - cbase]; else stu = fb_far_i32(J.stR + u);
            const double thru = fb_deep_cell1<FAR>(M, J, J.B, B, D, d + rs, rs, t, 2) + fb_score<ALL_LDS>(tab_lds, M.ltab, J.ltab, stt, stu, J.S) +
                                (double)M.r_lw[k1] + (double)M.c_lw[k2];            // VA:2269-2271
            if (do_x) fb_acc(bx, thru + J.l_ng);
            if (do_y) fb_acc(by, thru + J.l_ng);
            if (do_m) fb_acc(bm, thru + J.l_ng + J.l_ng);
        }
}

template <bool ALL_LDS>
__global__ __launch_bounds__(FB_RG_THREADS) void pg_fb_backward_deep(const PgFbJob *jobs) {
    __shared__ FbDeepSmem M;
    const PgFbJob J = jobs[blockIdx.x];
    const int tid = (int)threadIdx.x, nt = (int)blockDim.x;
    const double NI = ninf();
    const bool tab_lds = J.S * J.S <= 256;
    if (tab_lds) for (int k = tid; k < J.S * J.S; k += nt) M.ltab[k] = J.ltab[k];
    for (int k = tid; k < J.n_init && k < FB_RG_INIT; k += nt) { M.i_at[k] = J.init_at[k]; M.i_val[k] = J.init_val[k]; }
    const fb_gd Bm = (fb_gd)(unsigned long long)J.B;
    int seg = J.nseg, seg_lo = J.nd, B = 64, D = FB_DP_CELLS / 64, x = 0, drain = 0;
    bool live = false, do_x = false, do_y = false, do_m = false;
    int rbase = 0, cbase = 0, n_r = 0, n_c = 0;
    __syncthreads();
    for (int d = J.nd - 1; d >= 0; --d) {
        if (d < seg_lo) {
            --seg;
            const int sb = J.seg_B[seg];
            B = sb & 0xffff; D = FB_DP_CELLS / B; drain = (sb >> 16) ? (D / 2 - 1) : -1;
            seg_lo = J.seg_start[seg];
            FB_DEEP_WHO
            if (d < J.nd - 1) {
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __syncthreads();
                for (int dd = min(J.nd - 1, d + (D - 1)); dd > d; --dd) {
                    const int lo = J.imin[dd], n3 = 3 * (J.imax[dd] - lo + 1);
                    const double *src = J.B + 3 * J.doff[dd];
                    for (int k = tid; k < n3; k += nt) M.ring[((dd & (D - 1)) * 3 + k % 3) * B + ((lo + k / 3) & (B - 1))] = fb_far_ld(src + k);
                }
                __syncthreads();
            }
        }
        if (d == J.nd - 1 || (d & (FB_DP_REFILL - 1)) == FB_DP_REFILL - 1) {
            // the diagonals down to the next multiple of FB_DP_REFILL; their rows and columns (the smallest of either falls by at
            // most one a diagonal) with their forward lists, and the states up to FB_DP_HALO sites past the diagonal's last
            for (int k = tid; k < FB_DP_REFILL; k += nt) {
                const int dd = (d & ~(FB_DP_REFILL - 1)) + k;
                if (dd <= d) {
                    M.dmin[dd & (2 * FB_DP_REFILL - 1)] = J.imin[dd]; M.dmax[dd & (2 * FB_DP_REFILL - 1)] = J.imax[dd];
                    M.doff[k] = J.doff[dd]; M.dfar[k] = J.dfar[dd];
                }
            }
            const int mn_ = J.imin[d], mx_ = J.imax[d];
            rbase = max(0, mn_ - FB_DP_REFILL); cbase = max(0, d - mx_ - FB_DP_REFILL);
            n_r = min(min(J.Lx, mx_ + 1 + FB_DP_HALO) - rbase, FB_DP_W); n_c = min(min(J.Ly, d - mn_ + 1 + FB_DP_HALO) - cbase, FB_DP_W);
            const int e_r = J.foffL[rbase], e_c = J.foffR[cbase];
            const int n_er = min(J.foffL[rbase + n_r] - e_r, FB_DP_E), n_ec = min(J.foffR[cbase + n_c] - e_c, FB_DP_E);
            for (int k = tid; k <= n_r; k += nt) { M.r_off[k] = J.foffL[rbase + k] - e_r; if (k < n_r) M.r_st[k] = J.stL[rbase + k]; }
            for (int k = tid; k <= n_c; k += nt) { M.c_off[k] = J.foffR[cbase + k] - e_c; if (k < n_c) M.c_st[k] = J.stR[cbase + k]; }
            for (int k = tid; k < n_er; k += nt) { M.r_e[k] = J.fdstL[e_r + k]; M.r_lw[k] = J.flwL[e_r + k]; }
            for (int k = tid; k < n_ec; k += nt) { M.c_e[k] = J.fdstR[e_c + k]; M.c_lw[k] = J.flwR[e_c + k]; }
            fb_lds_barrier();
        }
        const int mn = M.dmin[d & (2 * FB_DP_REFILL - 1)], mx = M.dmax[d & (2 * FB_DP_REFILL - 1)];
        const int i = mn + ((x - mn) & (B - 1));
        if (live && i <= mx) {
            double bx = NI, by = NI, bm = NI;
            const long long at = M.doff[d & (FB_DP_REFILL - 1)] + (i - mn);
            if (d >= J.init_dmin)                                                   // initialise_array_corner_bwd, VA:740-854
                for (int k = 0; k < J.n_init; ++k) {
                    const long long w = M.i_at[k] - 3 * at;
                    if (w == 0) bx = M.i_val[k]; else if (w == 1) by = M.i_val[k]; else if (w == 2) bm = M.i_val[k];
                }
            if (M.dfar[d & (FB_DP_REFILL - 1)] & 2) {
                fb_deep_bwd_cell<ALL_LDS, true>(M, J, tab_lds, B, D, d, i, rbase, cbase, n_r, n_c, do_x, do_y, do_m, bx, by, bm);
            } else {
                asm volatile("s_nop 13" ::: "memory");
                fb_deep_bwd_cell<ALL_LDS, false>(M, J, tab_lds, B, D, d, i, rbase, cbase, n_r, n_c, do_x, do_y, do_m, bx, by, bm);
                asm volatile("s_nop 14" ::: "memory");
            }
            const fb_gd o = Bm + 3 * at;
            double *r = &M.ring[(d & (D - 1)) * 3 * B + x];
            if (do_x) { o[0] = bx; r[0] = bx; }
            if (do_y) { o[1] = by; r[B] = by; }
            if (do_m) { o[2] = bm; r[2 * B] = bm; }
        }
        if (drain >= 0 && (d & drain) == 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        fb_lds_barrier();
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) J.totals[1] = fb_far_rd(J, J.B, 0, 0, 2);
}
#undef FB_DEEP_WHO
