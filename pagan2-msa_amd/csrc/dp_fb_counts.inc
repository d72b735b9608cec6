// dp_fb_counts.inc -- the posterior over TRANSITIONS of a finished pagan_fb (included by dp_fb.hip, inside its anonymous
// namespace, behind dp_fb_post.inc): the expected number of times a path takes each arc of the forward recurrence, summed by
// the states at the arc's two ends (trans[3 * from + to]), the three end transitions, and for small alphabets the expected
// number of matches of each pair of character states (emit[a + b * S]).  These are the sufficient statistics of the pair model,
// and each count is the derivative of log_fwd by the matching log parameter (DESIGN.md s.6.5).
//
// An arc is one term of the forward recurrence with the weight the forward sweep gives it (pg_fb_forward): into X(i, j) from
// (p, j, X / Y / M) over the left bwd edges p -> i with l_ext / l_open / l_ng + l_open, into Y(i, j) the mirror over the right
// edges, into M(i, j) from (p, q, M / X / Y) over the edge pairs with 2 l_ng / l_ng / l_ng + ltab[a, b] + lwL + lwR.  Its share is
// xi = exp(F[pred] + log w + B[cell] - log_fwd), the argument clamped to <= 0 as fb_post clamps it; 0 where F or B is -inf,
// where the predecessor lies outside the band and where the full probability is 0.  The arcs into a cell sum to the cell's
// posterior.  Like the marginal passes this only READS F and B: no dependency between cells, a bandwidth kernel with about
// nine exps per simple cell.
//
// pg_fb_counts: a one-wave workgroup owns FB_CN_ROWS consecutive left rows, thread t row r0 + t, and walks anti-diagonals that
// cross its rows in ascending order (the lanes' own cells are one contiguous run of F and of B, as in pg_fb_marginals).  The
// diagonals that cross a row block are cut into segments of FB_CN_SEG and a workgroup takes ONE segment (the host lists them:
// a pair's work items, fb_counts_items): 64 rows of a full 2,000 x 2,000 matrix are 128,000 cells, and with a workgroup a row
// block the pass ran on fewer waves than the device has SIMDs.  The segment's intervals are staged in LDS with the FB_CN_HALO
// diagonals before it: most predecessors lie on those, and a predecessor further back is found with cell_at.  The row's left
// list is read once (its first entry stays in registers), the column's right list comes with the cell; the own cells of four
// diagonals are requested before the first of them is worked on.  A thread keeps its nine sums in registers, added in
// ascending j; the emission table is a column per lane of an LDS table [S][64] (a row has ONE left state, so b alone indexes
// it), folded over the lanes in lane order at the end.  No atomics anywhere: the workgroup's partial sums go to a scratch
// buffer and pg_fb_counts_fold adds them in work-item order -- the items depend on the pair alone --, so two runs, and a batch
// and a call per pair, give the same bits.  The end counts are one thread's walk over the end corner's terms in the forward
// sweep's order (fb_end_corner), each term as often as the forward total holds it.
#define FB_CN_ROWS 64
#define FB_CN_SEG 256             // diagonals of a work item
#define FB_CN_HALO 64
#define FB_CN_MAXS 32            // the emission table is provided up to this many character states (DNA)

struct PgFbCounts {
    double *part;                            // [n_items][9 + (emit ? S * S : 0)] the workgroups' partial sums
    double *out;                             // [12 + (emit ? S * S : 0)]: trans[12], then emit
    const int *items;                        // [n_items][3]: first row of the row block, first diagonal, last diagonal + 1
    int n_items;                             // work items of this pair (blockIdx.x beyond: nothing to do)
    int emit;                                // the emission table is wanted
};

__global__ __launch_bounds__(FB_CN_ROWS) void pg_fb_counts(const PgFbJob *jobs, const PgFbCounts *recs) {
    __shared__ int s_lo[FB_CN_HALO + FB_CN_SEG], s_hi[FB_CN_HALO + FB_CN_SEG];
    __shared__ long long s_base[FB_CN_HALO + FB_CN_SEG];
    __shared__ double s_fold[9][FB_CN_ROWS];
    __shared__ int s_st[FB_CN_ROWS];
    extern __shared__ double s_emit[];                             // [S][FB_CN_ROWS] when a pair of the launch wants the table
    const PgFbJob J = jobs[blockIdx.y];
    const PgFbCounts O = recs[blockIdx.y];
    if ((int)blockIdx.x >= O.n_items) return;                      // (a launch is as wide as its longest pair)
    const int r0 = O.items[3 * blockIdx.x], c = O.items[3 * blockIdx.x + 1], m = O.items[3 * blockIdx.x + 2] - c;   // m <= FB_CN_SEG
    const int r1 = min(J.Lx, r0 + FB_CN_ROWS) - 1, lane = (int)threadIdx.x, i = r0 + lane;
    const bool row = i <= r1;
    const double NI = ninf();
    const fb_gcd F = (fb_gcd)(unsigned long long)J.F, Bw = (fb_gcd)(unsigned long long)J.B;
    const double tot = J.totals[0];
    const bool live = tot > NI;                                    // (full probability 0: every count is 0)
    const bool emit = O.emit != 0;
    // the row's record: its left list (the first entry in registers) and its character state
    const bool rv = row && i > 0;
    const int l0 = rv ? J.offL[i] : 0, nl = rv ? J.offL[i + 1] - l0 : 0;
    const int p0 = nl > 0 ? J.srcL[l0] : 0;
    const double lwl0 = nl > 0 ? (double)J.lwL[l0] : 0.0;
    const int stl = rv ? J.stL[i] : -1;
    const double l_xx = J.l_ext, l_yx = J.l_open, l_mx = J.l_ng + J.l_open, l_mm = J.l_ng + J.l_ng, l_xm = J.l_ng;
    if (emit) for (int b = 0; b < J.S; ++b) s_emit[b * FB_CN_ROWS + lane] = 0.0;
    double nxx = 0.0, nxy = 0.0, nxm = 0.0, nyx = 0.0, nyy = 0.0, nym = 0.0, nmx = 0.0, nmy = 0.0, nmm = 0.0;
    auto share = [&](double f, double lw, double b) {
        const double x = f + lw + b - tot;
        return x > NI ? fb_exp_neg(fmin(x, 0.0)) : 0.0;
    };
    {
        const int sb = max(0, c - FB_CN_HALO);                     // the first diagonal staged
        for (int k = lane; k < c + m - sb; k += FB_CN_ROWS) {
            const int d = sb + k, mn = J.imin[d];
            s_lo[k] = mn; s_hi[k] = J.imax[d]; s_base[k] = J.doff[d] - mn;     // cell (p, d - p): base + p
        }
        __syncthreads();
        // the index of cell (p, q), 0 <= p < Lx, 0 <= q < Ly (a bwd edge's source), on a diagonal before c + m; -1 outside the band
        auto cell = [&](int p, int q) -> long long {
            const int d = p + q;
            if (d >= sb) return (p >= s_lo[d - sb] && p <= s_hi[d - sb]) ? s_base[d - sb] + p : -1;
            return cell_at(J, p, q);
        };
        for (int k = 0; k < m; k += 4) {
            double bx[4], by[4], bm[4], fmm[4];
            int ro[4], rn[4], str[4];
            bool act[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int kk = k + u, ix = c + kk - sb;            // (kk < FB_CN_SEG: k and the segment are multiples of 4)
                act[u] = live && kk < m && row && i >= s_lo[ix] && i <= s_hi[ix];
                bx[u] = by[u] = bm[u] = fmm[u] = NI;
                ro[u] = rn[u] = str[u] = 0;
                if (act[u]) {
                    const long long at = s_base[ix] + i;
                    bx[u] = Bw[3 * at]; by[u] = Bw[3 * at + 1]; bm[u] = Bw[3 * at + 2]; fmm[u] = F[3 * at + 2];
                    const int j = c + kk - i;
                    if (j > 0) { ro[u] = J.offR[j]; rn[u] = J.offR[j + 1] - ro[u]; str[u] = J.stR[j]; }
                }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (!act[u]) continue;
                const int j = c + k + u - i;
                if (bx[u] > NI)                                    // arcs into X(i, j): VA:2153, 2184, 2215
                    for (int e = 0; e < nl; ++e) {
                        const long long at = cell(e == 0 ? p0 : J.srcL[l0 + e], j);
                        if (at < 0) continue;
                        const double fx = F[3 * at], fy = F[3 * at + 1], fm = F[3 * at + 2];
                        nxx += share(fx, l_xx, bx[u]); nyx += share(fy, l_yx, bx[u]); nmx += share(fm, l_mx, bx[u]);
                    }
                if (by[u] > NI)                                    // arcs into Y(i, j)
                    for (int e = 0; e < rn[u]; ++e) {
                        const long long at = cell(i, J.srcR[ro[u] + e]);
                        if (at < 0) continue;
                        const double fx = F[3 * at], fy = F[3 * at + 1], fm = F[3 * at + 2];
                        nyy += share(fy, l_xx, by[u]); nxy += share(fx, l_yx, by[u]); nmy += share(fm, l_mx, by[u]);
                    }
                if (nl > 0 && rn[u] > 0) {                         // arcs into M(i, j): VA:2051, 2080, 2108 with the factors of :1383-1391
                    if (bm[u] > NI) {
                        const double sc = ((fb_gcd)(unsigned long long)J.ltab)[stl + (long long)str[u] * J.S];
                        for (int e1 = 0; e1 < nl; ++e1) {
                            const int p = e1 == 0 ? p0 : J.srcL[l0 + e1];
                            const double lwl = e1 == 0 ? lwl0 : (double)J.lwL[l0 + e1];
                            for (int e2 = 0; e2 < rn[u]; ++e2) {
                                const long long at = cell(p, J.srcR[ro[u] + e2]);
                                if (at < 0) continue;
                                const double w = sc + (lwl + (double)J.lwR[ro[u] + e2]);
                                const double fx = F[3 * at], fy = F[3 * at + 1], fm = F[3 * at + 2];
                                nmm += share(fm, l_mm + w, bm[u]); nxm += share(fx, l_xm + w, bm[u]); nym += share(fy, l_xm + w, bm[u]);
                            }
                        }
                    }
                    if (emit) s_emit[str[u] * FB_CN_ROWS + lane] += fb_post(fmm[u], bm[u], tot);
                }
            }
        }
    }
    // the workgroup's partial sums: over the lanes in lane order
    s_fold[0][lane] = nxx; s_fold[1][lane] = nxy; s_fold[2][lane] = nxm;
    s_fold[3][lane] = nyx; s_fold[4][lane] = nyy; s_fold[5][lane] = nym;
    s_fold[6][lane] = nmx; s_fold[7][lane] = nmy; s_fold[8][lane] = nmm;
    s_st[lane] = stl;
    __syncthreads();
    const int stride = 9 + (emit ? J.S * J.S : 0);
    double *part = O.part + (long long)blockIdx.x * stride;
    if (lane < 9) {
        double s = 0.0;
        for (int l = 0; l < FB_CN_ROWS; ++l) s += s_fold[lane][l];
        part[lane] = s;
    }
    if (emit)
        for (int e = lane; e < J.S * J.S; e += FB_CN_ROWS) {
            const int a = e % J.S, b = e / J.S;                    // emit[a + b * S]: left state a, right state b
            double s = 0.0;
            for (int l = 0; l < FB_CN_ROWS; ++l) if (s_st[l] == a) s += s_emit[b * FB_CN_ROWS + l];
            part[9 + e] = s;
        }
}

// The second launch: a workgroup per pair adds the work items' partial sums in item order; its first thread takes the end counts.
__global__ __launch_bounds__(256) void pg_fb_counts_fold(const PgFbJob *jobs, const PgFbCounts *recs) {
    const PgFbJob J = jobs[blockIdx.x];
    const PgFbCounts O = recs[blockIdx.x];
    const int stride = 9 + (O.emit ? J.S * J.S : 0);
    for (int e = (int)threadIdx.x; e < stride; e += (int)blockDim.x) {
        double s = 0.0;
        for (int g = 0; g < O.n_items; ++g) s += O.part[(long long)g * stride + e];
        O.out[e < 9 ? e : e + 3] = s;
    }
    if (threadIdx.x != 0) return;
    // X-close, Y-close, M-end: the terms of fb_end_corner in its order (the Y-close of a non-first right edge once per left edge)
    double ex = 0.0, ey = 0.0, em = 0.0;
    const double tot = J.totals[0];
    const int l0 = J.offL[J.Lx], l1 = J.offL[J.Lx + 1], r0 = J.offR[J.Ly], r1 = J.offR[J.Ly + 1];
    if (tot > ninf() && l1 > l0 && r1 > r0) {
        auto end = [&](double lf) { const double x = lf - tot; return x > ninf() ? fb_exp_neg(fmin(x, 0.0)) : 0.0; };
        auto mt = [&](int k1, int k2) { em += end(rd(J.F, cell_at(J, J.srcL[k1], J.srcR[k2]), 2) + J.l_ng + (double)J.lwL[k1] + (double)J.lwR[k2]); };
        auto xc = [&](int k1) { ex += end(rd(J.F, cell_at(J, J.srcL[k1], J.Ly - 1), 0)); };
        auto yc = [&](int k2) { ey += end(rd(J.F, cell_at(J, J.Lx - 1, J.srcR[k2]), 1)); };
        mt(l0, r0); xc(l0); yc(r0);
        for (int k2 = r0 + 1; k2 < r1; ++k2) { mt(l0, k2); yc(k2); }
        for (int k1 = l0 + 1; k1 < l1; ++k1) {
            mt(k1, r0); xc(k1);
            for (int k2 = r0 + 1; k2 < r1; ++k2) { mt(k1, k2); yc(k2); }
        }
    }
    O.out[9] = ex; O.out[10] = ey; O.out[11] = em;
}
