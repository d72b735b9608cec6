// dp_fb_sample.inc -- included by dp_fb.hip, inside its anonymous namespace, behind dp_fb_post.inc: sample_new_path (VA:1193-1322)
// on the device, K paths per pair in one launch (pg_fb_sample), over the forward matrix where the sweeps left it.
//
// One sampled path is a chain of dependent loads -- the cell's edge lists, the predecessors' cells, the pick, the next cell --
// with nothing to run side by side; K paths are K independent chains.  Grid = (groups of 64 paths, pairs), a workgroup is one
// wave, lane p of group g owns path 64 g + p of its pair and walks it from the end corner to (0, 0) on its own: no atomics, no
// communication between lanes, no LDS beyond the pair's two records (a wave's lanes finish at different steps; the wave ends with
// its longest path).
//
// The step restates pagan_fb_sample_path (dp_fb.hip), which the host keeps: the predecessors of the current cell and state in
// the forward pass's candidate order -- a match cell: the k1 x k2 edge pairs, each contributing M, X, Y; a gap cell: the edges of
// the moving side, each contributing own state, other gap, M -- every log weight added left to right as the host writes it
// (F + ng + ng + sc + w; the file is compiled without contraction), the log terms taken from the job record (l_ext, l_open, l_ng,
// ltab: the host's logs, never one taken here).  The pick: the maximum, the total of exp(lw - hi), the first index whose running
// sum reaches total * u.  A cell outside the band reads as -inf.  A step with up to FS_KEEP predecessor cells (every step between
// two plain sequences has one) keeps their candidates in registers between the passes; one with more lists them again in each
// pass.  exp is the device library's: it differs from the host's in the last bits, which moves a pick only when total * u lies
// within a few ulp of a running sum.  The one place where the text differs from the host's: a match state takes its score from
// ltab, the host from log(score[...]) -- the same table entry, the log taken once at staging.
//
// The uniform numbers are not uploaded: u(path, s) = (mix(key ^ (s + (path << 32))) >> 11) / 2^53 with key = mix(mix(seed) ^ node)
// (pagan_sample_uniforms_path; s = 0 is the end corner's), computed where they are used.
//
// Outputs.  Per path and step one record (i, j, word), word = state | k1 << 4 | k2 << 18 as the host packs it: what
// pagan_internal_replay takes.  Trace layout: [group][step][lane of the group], a group of w = min(64, K - 64 g) paths holding
// w * max_steps records from record 64 g * max_steps on -- the lanes at one step write one contiguous run, K paths take exactly
// 12 K (Lx + Ly) bytes, and a single path (the tree walk's) is contiguous.  Per path a summary of FB_SUMMARY_INTS ints (dp_fb.hip names them): status
// (0 sampled, 1 full probability zero, 2 internal: no candidate, or more than Lx + Ly steps), the end cell (state, i, j, k1, k2),
// the step count, the counts of M, X and Y steps, and log_q = the sum over the picks, the end corner's included, of
// (lw_k - hi) - log(total) = log(exp(lw_k - hi) / total): the log posterior probability of the path.

struct PgFbSample {
    unsigned long long key;          // mix(mix(seed) ^ node)
    int n_paths, groups, max_steps;  // K, ceil(K / 64), Lx + Ly
    int pad;
    int *trace;                      // null: summaries only (PAGAN_SAMPLE_NO_TRACES)
    int *summary;                    // [n_paths][FB_SUMMARY_INTS]
};

typedef const __attribute__((address_space(1))) int *fs_gi;
typedef const __attribute__((address_space(1))) float *fs_gf;
typedef const __attribute__((address_space(1))) long long *fs_gl;
typedef __attribute__((address_space(1))) int *fs_go;

__device__ __forceinline__ unsigned long long fs_mix(unsigned long long x) {      // fb_splitmix64, for the device
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}
__device__ __forceinline__ double fs_uniform(unsigned long long key, int path, int s) {
    return (double)(fs_mix(key ^ ((unsigned long long)(unsigned)s + ((unsigned long long)(unsigned)path << 32))) >> 11) * (1.0 / 9007199254740992.0);
}

// the job record's arrays as loads from global memory (a generic pointer loaded from the record compiles to flat loads)
struct FsJob {
    int Lx, Ly, S;
    double ext, open, ng;
    fs_gi stL, offL, srcL, stR, offR, srcR, imin, imax;
    fs_gf lwL, lwR;
    fs_gl doff;
    fb_gcd ltab, F;
    // the three forward logs of cell (p, q); -inf outside the matrices or the band (pagan_fb::at)
    __device__ __forceinline__ void cell(int p, int q, double &f0, double &f1, double &f2) const {
        f0 = f1 = f2 = ninf();
        if (p < 0 || q < 0 || p >= Lx || q >= Ly) return;
        const int d = p + q, mn = imin[d];
        if (p < mn || p > imax[d]) return;
        const long long at = 3 * (doff[d] + (p - mn));
        f0 = F[at]; f1 = F[at + 1]; f2 = F[at + 2];
    }
};

__device__ __forceinline__ FsJob fs_job_of(const PgFbJob &J) {
    FsJob V;
    V.Lx = J.Lx; V.Ly = J.Ly; V.S = J.S; V.ext = J.l_ext; V.open = J.l_open; V.ng = J.l_ng;
    V.stL = (fs_gi)(unsigned long long)J.stL; V.offL = (fs_gi)(unsigned long long)J.offL; V.srcL = (fs_gi)(unsigned long long)J.srcL;
    V.stR = (fs_gi)(unsigned long long)J.stR; V.offR = (fs_gi)(unsigned long long)J.offR; V.srcR = (fs_gi)(unsigned long long)J.srcR;
    V.imin = (fs_gi)(unsigned long long)J.imin; V.imax = (fs_gi)(unsigned long long)J.imax;
    V.lwL = (fs_gf)(unsigned long long)J.lwL; V.lwR = (fs_gf)(unsigned long long)J.lwR; V.doff = (fs_gl)(unsigned long long)J.doff;
    V.ltab = (fb_gcd)(unsigned long long)J.ltab; V.F = (fb_gcd)(unsigned long long)J.F;
    return V;
}

// iterate_bwd_edges_for_sampled_end_corner (VA:1904-2025) in the host's order: fn(lw, state, i, j, k1, k2), -1 = no edge
template <class Fn>
__device__ __forceinline__ void fs_corner(const FsJob &J, Fn &&fn) {
    const int l0 = J.offL[J.Lx], l1 = J.offL[J.Lx + 1], r0 = J.offR[J.Ly], r1 = J.offR[J.Ly + 1];
    if (!(l1 > l0 && r1 > r0)) return;
    auto mt = [&](int k1, int k2) {
        const int p = J.srcL[k1], q = J.srcR[k2];
        double f0, f1, f2;
        J.cell(p, q, f0, f1, f2);
        fn(f2 + J.ng + (double)J.lwL[k1] + (double)J.lwR[k2], 2, p, q, k1 - l0, k2 - r0);
    };
    auto xc = [&](int k1) {
        const int p = J.srcL[k1];
        double f0, f1, f2;
        J.cell(p, J.Ly - 1, f0, f1, f2);
        fn(f0, 0, p, J.Ly - 1, k1 - l0, -1);
    };
    auto yc = [&](int k2) {
        const int q = J.srcR[k2];
        double f0, f1, f2;
        J.cell(J.Lx - 1, q, f0, f1, f2);
        fn(f1, 1, J.Lx - 1, q, -1, k2 - r0);
    };
    for (int k1 = l0; k1 < l1; ++k1)
        for (int k2 = r0; k2 < r1; ++k2) {
            // (l0, r0): match, X close, Y close; a later right edge: match, Y close; a later left edge's first: match, X close
            mt(k1, k2);
            if (k2 == r0) xc(k1);
            if (k2 > r0 || k1 == l0) yc(k2);
        }
}

// the predecessors of cell (i, j) in `state`, a cell of the matrices at a time: fn(lw[3], state[3], p, q, k1, k2)
template <class Fn>
__device__ __forceinline__ void fs_preds(const FsJob &J, int state, int i, int j, Fn &&fn) {
    const bool mvL = state != PAGAN_Y_MAT, mvR = state != PAGAN_X_MAT;      // the sides that move: both in a match
    const int a0 = mvL ? J.offL[i] : 0, a1 = mvL ? J.offL[i + 1] : 1;
    const int b0 = mvR ? J.offR[j] : 0, b1 = mvR ? J.offR[j + 1] : 1;
    double sc = 0.0;
    if (state == PAGAN_M_MAT) sc = J.ltab[J.stL[i] + (long long)J.stR[j] * J.S];
    for (int k1 = a0; k1 < a1; ++k1) {
        const int p = mvL ? J.srcL[k1] : i;
        const double wl = mvL ? (double)J.lwL[k1] : 0.0;
        for (int k2 = b0; k2 < b1; ++k2) {
            const int q = mvR ? J.srcR[k2] : j;
            double f0, f1, f2;
            J.cell(p, q, f0, f1, f2);
            double lw[3];
            int st[3];
            if (state == PAGAN_M_MAT) {
                const double w = wl + (double)J.lwR[k2];
                lw[0] = f2 + J.ng + J.ng + sc + w; st[0] = 2;
                lw[1] = f0 + J.ng + sc + w; st[1] = 0;
                lw[2] = f1 + J.ng + sc + w; st[2] = 1;
            } else if (state == PAGAN_X_MAT) {
                lw[0] = f0 + J.ext; st[0] = 0;
                lw[1] = f1 + J.open; st[1] = 1;
                lw[2] = f2 + J.ng + J.open; st[2] = 2;
            } else {
                lw[0] = f1 + J.ext; st[0] = 1;
                lw[1] = f0 + J.open; st[1] = 0;
                lw[2] = f2 + J.ng + J.open; st[2] = 2;
            }
            fn(lw, st, p, q, mvL ? k1 - a0 : 0, mvR ? k2 - b0 : 0);
        }
    }
}

// a predecessor cell's three candidates, kept in registers between the passes of a step: the first FS_KEEP cells of a step
// (every loop over them is unrolled, so the array is registers)
#ifndef FS_KEEP
#define FS_KEEP 4
#endif
struct FsCell {
    double lw[3];
    double e[3];                     // exp(lw - hi), from the pass that totals them (the pick's running sum adds the same numbers)
    int st[3], p, q, a, b;
};
// what a pick leaves behind
struct FsPick {
    double sum, lw;
    int state, i, j, k1, k2;
    bool found;
};
// the host's `while (sum < rv && k + 1 < n)`: the running sum takes every candidate up to the first that reaches rv; the last
// candidate stays chosen when none does
__device__ __forceinline__ void fs_take_e(FsPick &P, double rv, double e, double lw, int state, int i, int j, int k1, int k2) {
    if (P.found) return;
    P.sum += e;
    P.lw = lw; P.state = state; P.i = i; P.j = j; P.k1 = k1; P.k2 = k2;
    if (!(P.sum < rv)) P.found = true;
}
__device__ __forceinline__ void fs_take(FsPick &P, double rv, double hi, double lw, int state, int i, int j, int k1, int k2) {
    if (P.found) return;
    P.sum += exp(lw - hi);
    P.lw = lw; P.state = state; P.i = i; P.j = j; P.k1 = k1; P.k2 = k2;
    if (!(P.sum < rv)) P.found = true;
}

__global__ __launch_bounds__(64) void pg_fb_sample(const PgFbJob *jobs, const PgFbSample *recs) {
    // the pair's record, staged in LDS: its thirteen pointers and three logs are read from there where a step uses them (as
    // uniform values they took more scalar registers than a wave has, and were spilled)
    __shared__ FsJob J;
    __shared__ PgFbSample R;
    // a launch is as wide as its pair with the most groups.  (The C ABI gives every pair of a call the same n_paths, so today all
    // pairs have the launch's width and this never fires; the record carries the count per pair.)
    if ((int)blockIdx.x >= recs[blockIdx.y].groups) return;
    const int lane = (int)threadIdx.x, path = 64 * (int)blockIdx.x + lane;
    if (lane == 0) { J = fs_job_of(jobs[blockIdx.y]); R = recs[blockIdx.y]; }
    __syncthreads();
    if (path >= R.n_paths) return;
    const int width = min(64, R.n_paths - 64 * (int)blockIdx.x);   // paths of this group
    const fs_go trace = R.trace ? (fs_go)(unsigned long long)R.trace + 3 * (64ll * blockIdx.x * R.max_steps + lane) : (fs_go)0;
    const fs_go out = (fs_go)(unsigned long long)R.summary + (long long)FB_SUMMARY_INTS * path;
    const double NI = ninf();
    double log_q = 0.0, tot_prod = 1.0;
    int status = 0, steps = 0, n_m = 0, n_x = 0, n_y = 0;
    int state = 0, i = 0, j = 0;
    int e_state = 0, e_i = 0, e_j = 0, e_k1 = -1, e_k2 = -1;
    {   // the end corner
        double hi = NI, tot = 0.0;
        fs_corner(J, [&](double lw, int, int, int, int, int) { hi = fmax(hi, lw); });
        if (hi == NI) {
            status = 1;                                            // full probability 0: nothing to sample
        } else {
            fs_corner(J, [&](double lw, int, int, int, int, int) { tot += exp(lw - hi); });
            const double rv = tot * fs_uniform(R.key, path, 0);
            FsPick P = {0.0, NI, 0, 0, 0, 0, 0, false};
            fs_corner(J, [&](double lw, int s, int p, int q, int a, int b) { fs_take(P, rv, hi, lw, s, p, q, a, b); });
            state = e_state = P.state; i = e_i = P.i; j = e_j = P.j; e_k1 = P.k1; e_k2 = P.k2;
            log_q += (P.lw - hi) - log(tot);
        }
    }
    while (status == 0 && !(i < 1 && j < 1)) {
        // pass 1: the maximum; the first FS_KEEP predecessor cells' candidates stay in registers (with 64 paths a wave, some lane
        // stands on a multi-edge site at most steps of a graph pair: a second and third listing then cost every lane of the wave)
        double hi = NI;
        FsCell c[FS_KEEP];
        int n_cells = 0;
        fs_preds(J, state, i, j, [&](const double *lw, const int *st, int p, int q, int a, int b) {
#pragma unroll
            for (int k = 0; k < FS_KEEP; ++k)
                if (n_cells == k) c[k] = FsCell{{lw[0], lw[1], lw[2]}, {0.0, 0.0, 0.0}, {st[0], st[1], st[2]}, p, q, a, b};
            hi = fmax(hi, fmax(lw[0], fmax(lw[1], lw[2])));
            ++n_cells;
        });
        if (hi == NI || steps >= R.max_steps) { status = 2; break; }
        const double u = fs_uniform(R.key, path, steps + 1);
        FsPick P = {0.0, NI, 0, 0, 0, 0, 0, false};
        double tot = 0.0;
        if (n_cells <= FS_KEEP) {
            // passes 2 and 3 over the kept cells
#pragma unroll
            for (int k = 0; k < FS_KEEP; ++k)
                if (k < n_cells)
                    for (int t = 0; t < 3; ++t) { c[k].e[t] = exp(c[k].lw[t] - hi); tot += c[k].e[t]; }
            const double rv = tot * u;
#pragma unroll
            for (int k = 0; k < FS_KEEP; ++k)
                if (k < n_cells)
                    for (int t = 0; t < 3; ++t) fs_take_e(P, rv, c[k].e[t], c[k].lw[t], c[k].st[t], c[k].p, c[k].q, c[k].a, c[k].b);
        } else {
            fs_preds(J, state, i, j, [&](const double *lw, const int *, int, int, int, int) {
                tot += exp(lw[0] - hi); tot += exp(lw[1] - hi); tot += exp(lw[2] - hi);
            });
            const double rv = tot * u;
            fs_preds(J, state, i, j, [&](const double *lw, const int *st, int p, int q, int a, int b) {
                fs_take(P, rv, hi, lw[0], st[0], p, q, a, b); fs_take(P, rv, hi, lw[1], st[1], p, q, a, b); fs_take(P, rv, hi, lw[2], st[2], p, q, a, b);
            });
        }
        // (lw_k - hi) - log(total): the totals' logs are taken 32 steps at a time, off the step's instruction stream (a total lies in
        // [1, 3 k1 k2]: the product of 32 is far from the range's end)
        log_q += P.lw - hi;
        tot_prod *= tot;
        if ((steps & 31) == 31) { log_q -= log(tot_prod); tot_prod = 1.0; }
        if (trace) {
            const fs_go t = trace + 3ll * steps * width;
            t[0] = i; t[1] = j; t[2] = (int)((unsigned)state | ((unsigned)P.k1 << 4) | ((unsigned)P.k2 << 18));
        }
        ++steps;
        n_m += state == PAGAN_M_MAT; n_x += state == PAGAN_X_MAT; n_y += state == PAGAN_Y_MAT;
        state = P.state; i = P.i; j = P.j;
    }
    log_q -= log(tot_prod);
    out[FB_SUM_STATUS] = status;
    out[FB_SUM_END] = e_state; out[FB_SUM_END + 1] = e_i; out[FB_SUM_END + 2] = e_j; out[FB_SUM_END + 3] = e_k1; out[FB_SUM_END + 4] = e_k2;
    out[FB_SUM_STEPS] = steps; out[FB_SUM_M] = n_m; out[FB_SUM_X] = n_x; out[FB_SUM_Y] = n_y;
    const long long lq = __double_as_longlong(log_q);
    out[FB_SUM_VALUE] = (int)(unsigned)(lq & 0xffffffffll); out[FB_SUM_VALUE + 1] = (int)(unsigned)((unsigned long long)lq >> 32);
    out[12] = out[13] = out[14] = out[15] = 0;
}

// one path's records out of its group's step-major block into a contiguous run (what pagan_internal_replay reads)
__global__ __launch_bounds__(256) void pg_fb_trace_pack(const int *group, int width, int lane, int n_steps, int *dst) {
    for (int t = (int)(blockIdx.x * blockDim.x + threadIdx.x); t < n_steps; t += (int)(gridDim.x * blockDim.x)) {
        const int *r = group + 3 * ((long long)t * width + lane);
        dst[3 * t] = r[0]; dst[3 * t + 1] = r[1]; dst[3 * t + 2] = r[2];
    }
}
