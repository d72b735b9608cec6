// dp_fb_post.inc -- what a caller reads out of a finished pagan_fb without taking the matrices to the host (included by dp_fb.hip,
// inside its anonymous namespace, behind the sweeps): the posterior of a list of cells (a path's support), and the posterior
// matrix reduced over rows and over columns (site marginals).  Both only READ the stored F / B arrays ([cell][X, Y, M],
// diagonal-major) and the pair's log full probability (totals[0], on the device since the forward sweep's end corner); there is
// no dependency between cells, so unlike the sweeps these are bandwidth kernels.
//
// post(s, i, j) = exp(F + B - log_fwd) (compute_posterior_score, VA:1029-1034), with the sweeps' own exp and the argument clamped
// to <= 0 (rounding may leave F + B a few ulp above log_fwd; a probability is not above 1).  A cell no path reaches (F or B
// is -inf) has posterior exactly 0, and so has every cell when the full probability itself is 0.

__device__ __forceinline__ double fb_post(double f, double b, double tot) {
    const double x = f + b - tot;
    return x > ninf() ? fb_exp_neg(fmin(x, 0.0)) : 0.0;             // (NaN -- -inf minus -inf -- compares false: 0)
}

// (a) gather.  One launch serves the cell lists of several pairs: blockIdx.y = pair, its record names the list and the output.
// cells: (state, i, j) triples; a state outside 0..2 (a skip column, pagan_path_cells) gives -1, a cell outside the band 0.
struct PgFbGather {
    const int *cells; double *out; int n;
};
__global__ __launch_bounds__(256) void pg_fb_gather(const PgFbJob *jobs, const PgFbGather *recs) {
    const PgFbJob J = jobs[blockIdx.y];
    const PgFbGather G = recs[blockIdx.y];
    const double tot = J.totals[0];
    for (long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x; k < G.n; k += (long long)gridDim.x * blockDim.x) {
        const int s = G.cells[3 * k], i = G.cells[3 * k + 1], j = G.cells[3 * k + 2];
        double p = -1.0;
        if (s >= 0 && s <= 2) {
            const long long at = cell_at(J, i, j);
            p = at < 0 ? 0.0 : fb_post(J.F[3 * at + s], J.B[3 * at + s], tot);
        }
        G.out[k] = p;
    }
}

// (b) site marginals.  Row pass (COL = false): a workgroup owns FB_PM_ROWS consecutive left rows, thread t row r0 + t, and walks the
// anti-diagonals that cross the block in ascending order; on diagonal d the lanes' cells lie at doff[d] + (i - imin[d]): consecutive
// cells, 24 B apart, in F and in B -- a wave's loads are one contiguous run.  A thread adds its row's post(X) and post(M) in
// registers in ascending j and keeps the largest post(M) (strictly larger replaces: ties stay with the lowest j; nothing above 0: -1).
// Column pass (COL = true): the mirror -- thread t holds right column c0 + t, its cell on diagonal d is doff[d] + (d - j - imin[d])
// (consecutive columns: consecutive cells, descending), sums post(Y) and post(M) in ascending i.  No atomics, no cross-lane sums:
// a site's result is one thread's sequence of additions, the same on every run.
//
// The diagonals of a block: the rows of diagonal d are [imin[d], imax[d]], its columns [d - imax[d], d - imin[d]], and for a
// monotone band all four bounds never fall as d grows (dp_band.h), so the first diagonal that reaches the block and the first
// beyond it are two binary searches.  The intervals and offsets are staged FB_PM_CHUNK diagonals at a time in LDS, and a
// thread issues the loads of four diagonals before it takes their exps, so that several runs are in flight per wave.
// FB_PM_ROWS = 64 (DESIGN.md s.6): one wave a workgroup.  A tunnel's diagonal holds 25-60 cells, so a taller block would only add
// waves without a cell on most diagonals; 64 lanes x 24 B is already 12 whole cache lines per load; and a full 700 x 700 matrix
// still spreads over 11 workgroups a pair.
#define FB_PM_ROWS 64
#define FB_PM_CHUNK 256
struct PgFbMarg {
    double *gap, *match, *best_p;            // [Lx]: pX, pM, best_p (rows) / [Ly]: pY, pM', best_p' (columns)
    int *best;                               // best_j / best_i
};
template <bool COL>
__global__ __launch_bounds__(FB_PM_ROWS) void pg_fb_marginals(const PgFbJob *jobs, const PgFbMarg *outs) {
    __shared__ int s_lo[FB_PM_CHUNK], s_hi[FB_PM_CHUNK];
    __shared__ long long s_base[FB_PM_CHUNK];
    const PgFbJob J = jobs[blockIdx.y];
    const PgFbMarg O = outs[blockIdx.y];
    const int n = COL ? J.Ly : J.Lx;
    const int r0 = (int)blockIdx.x * FB_PM_ROWS;
    if (r0 >= n) return;                                           // (a launch is as wide as its longest pair)
    const int r1 = min(n, r0 + FB_PM_ROWS) - 1, lane = (int)threadIdx.x, r = r0 + lane;
    int d_first, d_end;
    {
        int a = 0, b = J.nd;                                       // the first diagonal whose last row (column) is >= r0
        while (a < b) {
            const int mid = (a + b) >> 1;
            const int hi = COL ? mid - J.imin[mid] : J.imax[mid];
            if (hi >= r0) b = mid; else a = mid + 1;
        }
        d_first = a;
        b = J.nd;                                                  // the first diagonal whose first row (column) is > r1
        while (a < b) {
            const int mid = (a + b) >> 1;
            const int lo = COL ? mid - J.imax[mid] : J.imin[mid];
            if (lo > r1) b = mid; else a = mid + 1;
        }
        d_end = a;
    }
    const int G = COL ? PAGAN_Y_MAT : PAGAN_X_MAT;
    const fb_gcd F = (fb_gcd)(unsigned long long)J.F, Bw = (fb_gcd)(unsigned long long)J.B;
    const double tot = J.totals[0];
    double sg = 0.0, sm = 0.0, bp = 0.0;
    int bi = -1;
    for (int c = d_first; c < d_end; c += FB_PM_CHUNK) {
        const int m = min(FB_PM_CHUNK, d_end - c);
        for (int k = lane; k < m; k += FB_PM_ROWS) {
            const int d = c + k, mn = J.imin[d], mx = J.imax[d];
            const long long off = J.doff[d];
            s_lo[k] = COL ? d - mx : mn; s_hi[k] = COL ? d - mn : mx;
            s_base[k] = COL ? off + (d - mn) : off - mn;           // the thread's cell: base + r (rows), base - r (columns)
        }
        __syncthreads();
        for (int k = 0; k < m; k += 4) {
            double fg[4], bg[4], fm[4], bm[4];
            bool act[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int kk = k + u;                              // (< FB_PM_CHUNK: k and the chunk are multiples of 4)
                act[u] = kk < m && r <= r1 && r >= s_lo[kk] && r <= s_hi[kk];
                fg[u] = bg[u] = fm[u] = bm[u] = ninf();
                if (act[u]) {
                    const long long at = COL ? s_base[kk] - r : s_base[kk] + r;
                    fg[u] = F[3 * at + G]; bg[u] = Bw[3 * at + G];
                    fm[u] = F[3 * at + PAGAN_M_MAT]; bm[u] = Bw[3 * at + PAGAN_M_MAT];
                }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (act[u]) {
                    const double pm = fb_post(fm[u], bm[u], tot);
                    sg += fb_post(fg[u], bg[u], tot);
                    sm += pm;
                    if (pm > bp) { bp = pm; bi = c + k + u - r; }
                }
        }
        __syncthreads();                                           // (the next chunk overwrites the staging arrays)
    }
    if (r <= r1) { O.gap[r] = sg; O.match[r] = sm; O.best_p[r] = bp; O.best[r] = bi; }
}
