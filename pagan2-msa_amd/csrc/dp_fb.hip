// dp_fb.hip -- forward/backward sum-product over the three alignment matrices, posteriors, path sampling.
//
// Counterpart of the reference's `compute_full_score` pass (src/main/basic_alignment.h:621-625: --full-probability,
// --sample-path, --mpost-posterior-plot-file): the forward sums accumulated beside the Viterbi maxima
// (src/main/viterbi_alignment.cpp:2049-2054, 2078-2083, 2106-2111, 2151-2155, 2182-2186, 2213-2217, 2249-2253, with the
// factors of :1376-1393 and the end corner :1440-1552), the backward pass (:329-341, 740-854, 975-1026, 1571-1662,
// 2259-2305), the posterior (:1029-1034) and sample_new_path (:1193-1322, 1666-2025, 2309-2446).
//
// The reference multiplies raw probabilities, which under- and overflows beyond a few hundred columns; here every
// quantity is a logarithm (product = sum, sum = log-sum-exp in fp64).  Same cell layout as the Viterbi kernels
// (diagonal-major, [cell][X, Y, M]), same anti-diagonal wavefront: forward sweeps d = 0 .. nd-1 reading predecessor
// cells through the bwd edge lists, backward sweeps d = nd-1 .. 0 reading successor cells through the fwd edge lists
// (built on the host from the bwd CSR: a site's fwd list is its outgoing edges in creation order).  Operands in HBM/L2.
// Schedule: an alignment whose diagonals are narrow (a band) is one workgroup with a __syncthreads() per anti-diagonal;
// a wide one (round 4) is cut into 64 x 64 blocks that a grid of one-wave workgroups works through block anti-diagonal by
// block anti-diagonal (see pg_fb_forward_tiled below).  The sums here need to agree with the reference's to 1e-9, not bit
// for bit (log-sum-exp in place of its products), so unlike the Viterbi kernels nothing constrains the order of evaluation.
//
// Reference quirks kept (see oracle/oracle_fb.cpp, which restates the same rules on the CPU): full-probability terms
// use gap_ext for every gap (no end-gap extension) and the plain gap-open probability; edge weights enter matches only;
// the end corner visits the Y-close term of a non-first right edge once per left edge.  Cells outside the tunnel hold
// probability 0.
//
// What a pair runs on is not decided here: dp_fb_plan.cpp (plain C++, no HIP) reads the PAGAN_FB_* switches (FbSwitches) and plans a
// pair (fb_plan_pair -> FbPlan: band index, corner initialisation, forward lists, schedule, deep-ring segments, workgroup sizes,
// decode route); dp_fb_plan.h also holds PgFbJob and the constants plan and kernels share.  This file stages and launches the plan.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <condition_variable>
#include <memory>
#include <mutex>
#include <optional>
#include <thread>
#include <vector>

#include "../../include/pagan_dp.h"
#include "dp_band.h"
#include "dp_fb_plan.h"
#include "dp_hip.h"

using namespace fbplan;
using namespace pgdev;

namespace {

#define FB_TRY(expr) PG_HIP_CODE(expr, "pagan_fb", PAGAN_E_NODEVICE)

// a call that answers with a PAGAN_* code of its own
#define FB_DO(call) do { const int rc_ = (call); if (rc_ != PAGAN_OK) return rc_; } while (0)

__device__ __forceinline__ double ninf() { return -__builtin_huge_val(); }

// The sums' transcendental functions.  A log-sum-exp only ever asks for exp(x) with x <= 0 and for log(z) with
// 1 <= z <= 3 (the largest term factored out, at most two more), and it needs them to ~1e-16 ABSOLUTE: the library's
// exp / log1p -- correct to an ulp over their whole domain, special cases and all -- were ~3,000 of the instructions of a
// cell (the sweep's chain is latency of exactly these).  Here: exp by the usual reduction x = n ln2 + r and a degree-13
// Taylor polynomial in r (|r| <= 0.347: remainder 4e-18), log by z = 2^k m, m in (0.707, 1.415], s = (m - 1) / (m + 1),
// log m = 2 atanh s as a polynomial of degree 11 in s^2 (s^2 <= 0.0295: remainder 6e-19).  fma() explicitly: the file is
// compiled without contraction.
__device__ __forceinline__ double fb_exp_neg(double x) {
    x = fmax(x, -60.0);                                            // (e^-60 = 9e-27 beside a term of 1: nothing; and no -inf - -inf below)
    const double n = rint(x * 1.4426950408889634074);
    double r = fma(-n, 6.93147180369123816490e-01, x);
    r = fma(-n, 1.90821492927058770002e-10, r);
    double p = 1.6059043836821613e-10;                             // 1/13!
    p = fma(p, r, 2.08767569878681e-09);  p = fma(p, r, 2.505210838544172e-08); p = fma(p, r, 2.755731922398589e-07);
    p = fma(p, r, 2.755731922398589e-06); p = fma(p, r, 2.48015873015873e-05);  p = fma(p, r, 1.984126984126984e-04);
    p = fma(p, r, 1.388888888888889e-03); p = fma(p, r, 8.333333333333333e-03); p = fma(p, r, 4.1666666666666664e-02);
    p = fma(p, r, 1.6666666666666666e-01); p = fma(p, r, 0.5); p = fma(p, r, 1.0); p = fma(p, r, 1.0);
    return ldexp(p, (int)n);
}
__device__ __forceinline__ double fb_log_1to3(double z) {
    const bool k1 = z > 1.4142135623730951, k2 = z > 2.8284271247461903;
    const double m = k2 ? 0.25 * z : (k1 ? 0.5 * z : z);
    const double kl = k2 ? 1.3862943611198906 : (k1 ? 0.6931471805599453 : 0.0);
    const double den = m + 1.0;
    double y = __builtin_amdgcn_rcp(den);
    y = fma(fma(-den, y, 1.0), y, y);
    y = fma(fma(-den, y, 1.0), y, y);
    const double num = m - 1.0;
    double sq = num * y;
    sq = fma(fma(-den, sq, num), y, sq);                           // one more correction of the quotient itself
    const double w = sq * sq;
    double p = 1.0 / 23.0;
    p = fma(p, w, 1.0 / 21.0); p = fma(p, w, 1.0 / 19.0); p = fma(p, w, 1.0 / 17.0); p = fma(p, w, 1.0 / 15.0);
    p = fma(p, w, 1.0 / 13.0); p = fma(p, w, 1.0 / 11.0); p = fma(p, w, 1.0 / 9.0);  p = fma(p, w, 1.0 / 7.0);
    p = fma(p, w, 1.0 / 5.0);  p = fma(p, w, 1.0 / 3.0);  p = fma(p, w, 1.0);
    return fma(2.0 * sq, p, kl);
}

// log(exp(a) + exp(b))
__device__ __forceinline__ double lse(double a, double b) {
    const double hi = fmax(a, b), lo = fmin(a, b);
    if (hi == ninf()) return hi;
    return hi + fb_log_1to3(1.0 + fb_exp_neg(lo - hi));
}

// log(exp(a) + exp(b) + exp(c)): the largest term is factored out, the other two cost an exp each
__device__ __forceinline__ double lse3(double a, double b, double c) {
    const double hi = fmax(a, fmax(b, c));
    if (hi == ninf()) return hi;
    // the two that are not the (first) largest
    const double u = a == hi ? b : a, v = (a == hi || b == hi) ? c : b;
    return hi + fb_log_1to3(1.0 + (fb_exp_neg(u - hi) + fb_exp_neg(v - hi)));
}

// The model's log score: from the LDS copy when the table fits (S * S <= 256), else from memory -- as two loads in two address
// spaces behind a uniform branch.  Written as `tab_lds ? M.ltab[k] : J.ltab[k]` the compiler selects the POINTER and emits one
// flat load, and a flat load is a vector memory operation: s_waitcnt vmcnt(0) behind it waited for the wave's stores of the step
// before, on every step of every sweep.
typedef const __attribute__((address_space(1))) double *fb_gcd;
// ALL_LDS: the launch holds only pairs whose table is in LDS, and the load from memory is not even compiled: with both paths in one
// kernel the LDS read still waited -- s_waitcnt vmcnt(0): the wave's stores of the step before -- because its destination register
// is the memory load's too, and the compiler cannot know that load was never issued.
template <bool ALL_LDS>
__device__ __forceinline__ double fb_score(bool tab_lds, const double *lds_tab, const double *mem_tab, int a, int b, int S) {
    if (ALL_LDS || tab_lds) return lds_tab[a + b * S];
    return ((fb_gcd)(unsigned long long)mem_tab)[a + (long long)b * S];
}

__device__ __forceinline__ long long cell_at(const PgFbJob &J, int p, int q) {
    if (p < 0 || q < 0 || p >= J.Lx || q >= J.Ly) return -1;
    const int d = p + q;
    const int mn = J.imin[d], mx = J.imax[d];
    return (p >= mn && p <= mx) ? J.doff[d] + (p - mn) : -1;
}

__device__ __forceinline__ double rd(const double *A, long long at, int s) { return at >= 0 ? A[3 * at + s] : ninf(); }

// The end corner, VA:1440-1552, behind a forward sweep: what the end site's edge lists reach, in the reference's order (the Y-close term
// of a non-first right edge once per left edge).  cell(p, q, s): the log forward score of state s of cell (p, q), -inf outside the band.
template <class Cell>
__device__ __forceinline__ double fb_end_corner(const PgFbJob &J, Cell cell) {
    double acc = ninf();
    const int l0 = J.offL[J.Lx], l1 = J.offL[J.Lx + 1], r0 = J.offR[J.Ly], r1 = J.offR[J.Ly + 1];
    auto mt = [&](int k1, int k2) { return cell(J.srcL[k1], J.srcR[k2], 2) + J.l_ng + (double)J.lwL[k1] + (double)J.lwR[k2]; };
    auto xc = [&](int k1) { return cell(J.srcL[k1], J.Ly - 1, 0); };
    auto yc = [&](int k2) { return cell(J.Lx - 1, J.srcR[k2], 1); };
    if (l1 > l0 && r1 > r0) {
        acc = lse(acc, mt(l0, r0)); acc = lse(acc, xc(l0)); acc = lse(acc, yc(r0));
        for (int k2 = r0 + 1; k2 < r1; ++k2) { acc = lse(acc, mt(l0, k2)); acc = lse(acc, yc(k2)); }
        for (int k1 = l0 + 1; k1 < l1; ++k1) {
            acc = lse(acc, mt(k1, r0)); acc = lse(acc, xc(k1));
            for (int k2 = r0 + 1; k2 < r1; ++k2) { acc = lse(acc, mt(k1, k2)); acc = lse(acc, yc(k2)); }
        }
    }
    return acc;
}

__global__ __launch_bounds__(1024) void pg_fb_forward(const PgFbJob *jobs) {
    const PgFbJob J = jobs[blockIdx.x];
    for (int d = 0; d < J.nd; ++d) {
        const int mn = J.imin[d], mx = J.imax[d];
        const long long off = J.doff[d];
        for (int i = mn + (int)threadIdx.x; i <= mx; i += (int)blockDim.x) {
            const int j = d - i;
            double fx = ninf(), fy = ninf(), fm = ninf();
            if (i == 0 && j == 0) {
                fm = 0.0;                                                          // fwd_score = 1, VA:730
            } else {
                if (i > 0)
                    for (int k = J.offL[i]; k < J.offL[i + 1]; ++k) {
                        const long long at = cell_at(J, J.srcL[k], j);
                        fx = lse(fx, lse3(rd(J.F, at, 0) + J.l_ext,                 // VA:2153
                                          rd(J.F, at, 1) + J.l_open,                // VA:2184 (gap_close = 1)
                                          rd(J.F, at, 2) + J.l_ng + J.l_open));     // VA:2215
                    }
                if (j > 0)
                    for (int k = J.offR[j]; k < J.offR[j + 1]; ++k) {
                        const long long at = cell_at(J, i, J.srcR[k]);
                        fy = lse(fy, lse3(rd(J.F, at, 1) + J.l_ext, rd(J.F, at, 0) + J.l_open, rd(J.F, at, 2) + J.l_ng + J.l_open));
                    }
                if (i > 0 && j > 0) {
                    const double sc = J.ltab[J.stL[i] + (long long)J.stR[j] * J.S];
                    const double mm = J.l_ng + J.l_ng + sc, xm = J.l_ng + sc;      // VA:1383-1391
                    for (int k1 = J.offL[i]; k1 < J.offL[i + 1]; ++k1)
                        for (int k2 = J.offR[j]; k2 < J.offR[j + 1]; ++k2) {
                            const long long at = cell_at(J, J.srcL[k1], J.srcR[k2]);
                            const double w = (double)J.lwL[k1] + (double)J.lwR[k2];
                            fm = lse(fm, lse3(rd(J.F, at, 2) + mm + w,              // VA:2051
                                              rd(J.F, at, 0) + xm + w,              // VA:2080
                                              rd(J.F, at, 1) + xm + w));            // VA:2108
                        }
                }
            }
            double *o = J.F + 3 * (off + (i - mn));
            o[0] = fx; o[1] = fy; o[2] = fm;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0)
        J.totals[0] = fb_end_corner(J, [&](int p, int q, int s_) { return rd(J.F, cell_at(J, p, q), s_); });
}

__global__ __launch_bounds__(1024) void pg_fb_backward(const PgFbJob *jobs) {
    const PgFbJob J = jobs[blockIdx.x];
    for (long long k = threadIdx.x; k < 3 * J.cells; k += blockDim.x) J.B[k] = ninf();
    __syncthreads();
    for (int k = threadIdx.x; k < J.n_init; k += blockDim.x) J.B[J.init_at[k]] = J.init_val[k];   // VA:740-854
    __syncthreads();
    for (int d = J.nd - 1; d >= 0; --d) {
        const int mn = J.imin[d], mx = J.imax[d];
        const long long off = J.doff[d];
        for (int i = mn + (int)threadIdx.x; i <= mx; i += (int)blockDim.x) {
            const int j = d - i;
            double *o = J.B + 3 * (off + (i - mn));
            double bx = o[0], by = o[1], bm = o[2];
            for (int k = J.foffL[i]; k < J.foffL[i + 1]; ++k) {                    // iterate_fwd_edges_for_gap, left site
                const int t = J.fdstL[k];
                if (t >= J.Lx) continue;                                           // VA:1580
                const double nx = rd(J.B, cell_at(J, t, j), 0);
                bx = lse(bx, nx + J.l_ext); by = lse(by, nx + J.l_open); bm = lse(bm, nx + J.l_ng + J.l_open);   // VA:2281-2303
            }
            for (int k = J.foffR[j]; k < J.foffR[j + 1]; ++k) {
                const int t = J.fdstR[k];
                if (t >= J.Ly) continue;
                const double ny = rd(J.B, cell_at(J, i, t), 1);
                by = lse(by, ny + J.l_ext); bx = lse(bx, ny + J.l_open); bm = lse(bm, ny + J.l_ng + J.l_open);
            }
            for (int k1 = J.foffL[i]; k1 < J.foffL[i + 1]; ++k1)                    // iterate_fwd_edges_for_match
                for (int k2 = J.foffR[j]; k2 < J.foffR[j + 1]; ++k2) {
                    const int t = J.fdstL[k1], u = J.fdstR[k2];
                    if (t >= J.Lx || u >= J.Ly) continue;
                    const double thru = rd(J.B, cell_at(J, t, u), 2) + J.ltab[J.stL[t] + (long long)J.stR[u] * J.S] +
                                        (double)J.flwL[k1] + (double)J.flwR[k2];   // VA:2269-2271
                    bx = lse(bx, thru + J.l_ng); by = lse(by, thru + J.l_ng); bm = lse(bm, thru + J.l_ng + J.l_ng);
                }
            o[0] = bx; o[1] = by; o[2] = bm;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) J.totals[1] = rd(J.B, cell_at(J, 0, 0), 2);
}

// ---- long tunnels between plain sequences: one workgroup, lane = row mod B, the last diagonals in an LDS ring ----
// (round 5, last session.)  The one-workgroup sweeps above pay a full __syncthreads() -- the wave's stores acknowledged -- and
// round trips to L2 for operands and list entries on every cell diagonal (2.7 us); the block schedule sweeps every cell diagonal
// of a tunnel twice, with 25 of 64 lanes at work, behind a counter barrier.  When every site of both graphs has exactly one edge,
// from the site before it (leaf sequences: what a tunnel of 2 x 100 kb is made of), a cell reads (i-1, j), (i, j-1) of the
// diagonal before and (i-1, j-1) of the one before that, and nothing else.  Thread x owns the row i = x (mod B) of the current
// diagonal (B = blockDim >= the widest diagonal: at most one such row), the last three diagonals live in LDS ([slot][state][x]; an
// idle thread writes -inf), an operand is a read of the neighbouring lane's slot -- valid if that row was in the band on that
// diagonal, which two compares against the diagonal's interval tell --, the rows' and the columns' records (state, log weight of
// the one edge) and the diagonals' intervals sit in LDS windows refilled every FB_RG_REFILL diagonals, and the step ends in
// s_waitcnt lgkmcnt(0) + s_barrier: the scores go to memory unwaited-for.  Graph pairs (any site with another edge
// list) inside a tunnel take the deep-ring sweeps of dp_fb_deep.inc; diagonals wider than 1,024 cells keep the block schedule.
#define FB_RG_COLS 1024          // columns / rows in the LDS windows (>= B + 2 * FB_RG_REFILL) up to B = 512; 2,048 for B = 1,024
#define FB_RG_REFILL 256
// Who a thread is.  A cell's three states are three independent log-sum-exps of the same size -- the step's latency is one wave's
// way through them --, so up to B = 256 a row has THREE threads, one per state (NSPLIT = 3, blockDim = 3 B), and with B = 512 two
// (NSPLIT = 2: X and Y in one, M in the other; 1,024 threads is what a workgroup holds): wave w works on part w % NSPLIT of the
// rows 64 (w / NSPLIT) ..., which puts the waves of a block of rows on different SIMDs (waves go to the SIMDs round-robin).
// NSPLIT is a template argument: with the parts as run-time flags the one-thread-per-row sweeps lost a third of their speed.
// x: the thread's row modulo B; do_x / do_y / do_m: its states; tid / nt: for the staging loops, which all threads share.
#define FB_RING_THREADS                                                                                       \
    const int tid = (int)threadIdx.x, nt = (int)blockDim.x;                                                   \
    const int B = nt / NSPLIT;                                                                                \
    const int part = (tid >> 6) % NSPLIT;                                                                     \
    const int x = ((tid >> 6) / NSPLIT) * 64 + (tid & 63);                                                    \
    const bool do_x = NSPLIT == 1 || part == 0, do_y = NSPLIT == 1 || (NSPLIT == 2 ? part == 0 : part == 1), \
               do_m = NSPLIT == 1 || part == NSPLIT - 1;
typedef __attribute__((address_space(1))) double *fb_gd;

__device__ __forceinline__ void fb_lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// Nothing on a step's path is a load from memory (a vector load would wait behind the wave's stores -- memory operations
// complete in order --, and the compiler cannot make scalar loads of arrays it has only a pointer from memory to): the diagonals'
// intervals and offsets, the rows' and the columns' records are staged every FB_RG_REFILL diagonals for the next FB_RG_REFILL.
// MAXB = 512: 59 KB.  MAXB = 1024 (one thread a row; round 5: a workgroup's LDS is not bounded by 64 KB on gfx950 --
// tools/ubench/lds_big.hip): a ring of 74 KB, windows of 2,048 rows / columns, 113 KB in all.
template <int MAXB>
struct FbRingSmem {
    static constexpr int COLS = MAXB > 512 ? 2048 : FB_RG_COLS;
    double ring[3][3][MAXB];           // [diagonal slot][X, Y, M][thread]
    int c_st[COLS]; float c_lw[COLS];      // column j at j % FB_RG_COLS: state, log weight of the edge (j-1) -> j
    int r_st[COLS]; float r_lw[COLS];      // row i the same way
    int dmin[FB_RG_REFILL], dmax[FB_RG_REFILL]; long long doff[FB_RG_REFILL];     // diagonal d at d % FB_RG_REFILL
    double ltab[256];
    long long i_at[FB_RG_INIT]; double i_val[FB_RG_INIT];                         // initialise_array_corner_bwd's assignments (backward sweep)
};

template <bool ALL_LDS, int NSPLIT, int MAXB>
__global__ __launch_bounds__(FB_RG_THREADS) void pg_fb_forward_ring(const PgFbJob *jobs) {
    __shared__ FbRingSmem<MAXB> M;
    constexpr int CMASK = FbRingSmem<MAXB>::COLS - 1;
    const PgFbJob J = jobs[blockIdx.x];
    FB_RING_THREADS
    const int xm1 = (x - 1) & (B - 1);
    const double NI = ninf();
    const bool tab_lds = J.S * J.S <= 256;
    if (tab_lds) for (int k = tid; k < J.S * J.S; k += nt) M.ltab[k] = J.ltab[k];
    for (int q = 0; q < 9; ++q) (&M.ring[0][0][0])[q * MAXB + x] = NI;
    int mn1 = 0, mx1 = -1, mn2 = 0, mx2 = -1;            // the intervals of the diagonals d-1, d-2
    int s0 = 0, s1 = 2, s2 = 1;                          // ring slots of d, d-1, d-2
    int cols_hi = -1, rows_hi = -1;                      // columns <= cols_hi, rows <= rows_hi are in the windows
    const fb_gd F = (fb_gd)(unsigned long long)J.F;
    __syncthreads();
    for (int d = 0; d < J.nd; ++d) {
        if ((d & (FB_RG_REFILL - 1)) == 0) {
            // the next FB_RG_REFILL diagonals; their columns and rows: the largest of either grows by at most one a diagonal
            for (int k = tid; k < FB_RG_REFILL; k += nt) {
                const int dd = d + k;
                const bool in = dd < J.nd;
                M.dmin[k] = in ? J.imin[dd] : 0; M.dmax[k] = in ? J.imax[dd] : -1; M.doff[k] = in ? J.doff[dd] : 0;
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
            fb_lds_barrier();                                      // (the staged values went through registers into LDS: the loads are done)
        }
        const int mn = M.dmin[d & (FB_RG_REFILL - 1)], mx = M.dmax[d & (FB_RG_REFILL - 1)];
        const int i = mn + ((x - mn) & (B - 1));
        const bool active = i <= mx;
        double fx = NI, fy = NI, fm = NI;
        if (active) {
            const int j = d - i;
            if (i == 0 && j == 0) {
                fm = 0.0;                                                          // fwd_score = 1, VA:730
            } else {
                if (do_x && i > 0 && i - 1 >= mn1 && i - 1 <= mx1) {               // (i-1, j): VA:2153, 2184, 2215
                    const double ax = M.ring[s1][0][xm1], ay = M.ring[s1][1][xm1], am = M.ring[s1][2][xm1];
                    fx = lse3(ax + J.l_ext, ay + J.l_open, am + J.l_ng + J.l_open);
                }
                if (do_y && j > 0 && i >= mn1 && i <= mx1) {                       // (i, j-1)
                    const double px = M.ring[s1][0][x], py = M.ring[s1][1][x], pm = M.ring[s1][2][x];
                    fy = lse3(py + J.l_ext, px + J.l_open, pm + J.l_ng + J.l_open);
                }
                if (do_m && i > 0 && j > 0 && i - 1 >= mn2 && i - 1 <= mx2) {      // (i-1, j-1): VA:2051, 2080, 2108
                    const double cx = M.ring[s2][0][xm1], cy = M.ring[s2][1][xm1], cm = M.ring[s2][2][xm1];
                    const int str = M.r_st[i & CMASK], stc = M.c_st[j & CMASK];
                    const double sc = fb_score<ALL_LDS>(tab_lds, M.ltab, J.ltab, str, stc, J.S);
                    const double w = (double)M.r_lw[i & CMASK] + (double)M.c_lw[j & CMASK];
                    const double mm = J.l_ng + J.l_ng + sc + w, xm = J.l_ng + sc + w;   // VA:1383-1391
                    fm = lse3(cm + mm, cx + xm, cy + xm);
                }
            }
            const fb_gd o = F + 3 * (M.doff[d & (FB_RG_REFILL - 1)] + (i - mn));
            if (do_x) o[0] = fx;
            if (do_y) o[1] = fy;
            if (do_m) o[2] = fm;
        }
        if (do_x) M.ring[s0][0][x] = fx;
        if (do_y) M.ring[s0][1][x] = fy;
        if (do_m) M.ring[s0][2][x] = fm;
        mn2 = mn1; mx2 = mx1; mn1 = mn; mx1 = mx;
        { const int t = s2; s2 = s1; s1 = s0; s0 = t; }
        fb_lds_barrier();
    }
    __syncthreads();                                                               // (the end corner reads the scores from memory)
    if (threadIdx.x == 0)
        J.totals[0] = fb_end_corner(J, [&](int p, int q, int s_) { return rd(J.F, cell_at(J, p, q), s_); });
}

// Mirrored: diagonals nd-1 .. 0; a cell reads (i+1, j), (i, j+1) of the diagonal after it and (i+1, j+1) of the one after that;
// the windows hold row t = i+1's and column u = j+1's records (state, weight of the edge from the site before).
// What initialise_array_corner_bwd assigns (a handful of cells on the last diagonals, VA:740-854) is laid over the -inf a cell
// starts from on the diagonals >= init_dmin, and there the sums are taken one by one as pg_fb_backward takes them.
template <bool ALL_LDS, int NSPLIT, int MAXB>
__global__ __launch_bounds__(FB_RG_THREADS) void pg_fb_backward_ring(const PgFbJob *jobs) {
    __shared__ FbRingSmem<MAXB> M;
    constexpr int CMASK = FbRingSmem<MAXB>::COLS - 1;
    const PgFbJob J = jobs[blockIdx.x];
    FB_RING_THREADS
    const int xp1 = (x + 1) & (B - 1);
    const double NI = ninf();
    const bool tab_lds = J.S * J.S <= 256;
    if (tab_lds) for (int k = tid; k < J.S * J.S; k += nt) M.ltab[k] = J.ltab[k];
    for (int q = 0; q < 9; ++q) (&M.ring[0][0][0])[q * MAXB + x] = NI;
    int mn1 = 0, mx1 = -1, mn2 = 0, mx2 = -1;            // the intervals of the diagonals d+1, d+2
    int s0 = 0, s1 = 2, s2 = 1;
    for (int k = tid; k < J.n_init && k < FB_RG_INIT; k += nt) { M.i_at[k] = J.init_at[k]; M.i_val[k] = J.init_val[k]; }   // (in LDS: no load from memory inside the sweep's loop but the staging's)
    int cols_lo = J.Ly, rows_lo = J.Lx;                  // columns >= cols_lo, rows >= rows_lo are in the windows
    const fb_gd Bm = (fb_gd)(unsigned long long)J.B;
    __syncthreads();
    for (int d = J.nd - 1; d >= 0; --d) {
        if (d == J.nd - 1 || (d & (FB_RG_REFILL - 1)) == FB_RG_REFILL - 1) {
            // the diagonals down to the next multiple of FB_RG_REFILL; columns u = j + 1 and rows t = i + 1: the smallest of either
            // falls by at most one a diagonal
            for (int k = tid; k < FB_RG_REFILL; k += nt) {
                const int dd = (d & ~(FB_RG_REFILL - 1)) + k;
                if (dd <= d) { M.dmin[k] = J.imin[dd]; M.dmax[k] = J.imax[dd]; M.doff[k] = J.doff[dd]; }
            }
            const int mn_ = J.imin[d], mx_ = J.imax[d];
            const int want_c = max(0, d - mx_ + 1 - FB_RG_REFILL), want_r = max(0, mn_ + 1 - FB_RG_REFILL);
            for (int u = cols_lo - 1 - tid; u >= want_c; u -= nt) {
                M.c_st[u & CMASK] = J.stR[u];
                M.c_lw[u & CMASK] = u > 0 ? J.lwR[u - 1] : 0.0f;
            }
            for (int t = rows_lo - 1 - tid; t >= want_r; t -= nt) {
                M.r_st[t & CMASK] = J.stL[t];
                M.r_lw[t & CMASK] = t > 0 ? J.lwL[t - 1] : 0.0f;
            }
            cols_lo = min(cols_lo, want_c); rows_lo = min(rows_lo, want_r);
            fb_lds_barrier();                                      // (the staged values went through registers into LDS: the loads are done)
        }
        const int mn = M.dmin[d & (FB_RG_REFILL - 1)], mx = M.dmax[d & (FB_RG_REFILL - 1)];
        const int i = mn + ((x - mn) & (B - 1));
        const bool active = i <= mx;
        double bx = NI, by = NI, bm = NI;
        if (active) {
            const int j = d - i;
            const bool has_a = i + 1 < J.Lx && i + 1 >= mn1 && i + 1 <= mx1;       // (i+1, j)
            const bool has_p = j + 1 < J.Ly && i >= mn1 && i <= mx1;               // (i, j+1)
            const bool has_c = i + 1 < J.Lx && j + 1 < J.Ly && i + 1 >= mn2 && i + 1 <= mx2;   // (i+1, j+1)
            const double nx = has_a ? M.ring[s1][0][xp1] : NI, ny = has_p ? M.ring[s1][1][x] : NI;
            double thru = NI;
            if (i + 1 < J.Lx && j + 1 < J.Ly) {
                const int str = M.r_st[(i + 1) & CMASK], stc = M.c_st[(j + 1) & CMASK];
                const double sc = fb_score<ALL_LDS>(tab_lds, M.ltab, J.ltab, str, stc, J.S);
                thru = (has_c ? M.ring[s2][2][xp1] : NI) + sc + (double)M.r_lw[(i + 1) & CMASK] + (double)M.c_lw[(j + 1) & CMASK];   // VA:2269-2271
            }
            const long long at = M.doff[d & (FB_RG_REFILL - 1)] + (i - mn);
            if (d >= J.init_dmin) {
                for (int k = 0; k < J.n_init; ++k) {
                    const long long w = M.i_at[k] - 3 * at;
                    if (w == 0) bx = M.i_val[k]; else if (w == 1) by = M.i_val[k]; else if (w == 2) bm = M.i_val[k];
                }
                // (one by one, as pg_fb_backward takes them; a state's sums do not look at the other states')
                if (i + 1 < J.Lx) { if (do_x) bx = lse(bx, nx + J.l_ext); if (do_y) by = lse(by, nx + J.l_open); if (do_m) bm = lse(bm, nx + J.l_ng + J.l_open); }   // VA:2281-2303
                if (j + 1 < J.Ly) { if (do_y) by = lse(by, ny + J.l_ext); if (do_x) bx = lse(bx, ny + J.l_open); if (do_m) bm = lse(bm, ny + J.l_ng + J.l_open); }
                if (i + 1 < J.Lx && j + 1 < J.Ly) { if (do_x) bx = lse(bx, thru + J.l_ng); if (do_y) by = lse(by, thru + J.l_ng); if (do_m) bm = lse(bm, thru + J.l_ng + J.l_ng); }
            } else {
                if (do_x) bx = lse3(nx + J.l_ext, ny + J.l_open, thru + J.l_ng);
                if (do_y) by = lse3(nx + J.l_open, ny + J.l_ext, thru + J.l_ng);
                if (do_m) bm = lse3(nx + J.l_ng + J.l_open, ny + J.l_ng + J.l_open, thru + J.l_ng + J.l_ng);
            }
            const fb_gd o = Bm + 3 * at;
            if (do_x) o[0] = bx;
            if (do_y) o[1] = by;
            if (do_m) o[2] = bm;
        }
        if (do_x) M.ring[s0][0][x] = bx;
        if (do_y) M.ring[s0][1][x] = by;
        if (do_m) M.ring[s0][2][x] = bm;
        mn2 = mn1; mx2 = mx1; mn1 = mn; mx1 = mx;
        { const int t = s2; s2 = s1; s1 = s0; s0 = t; }
        fb_lds_barrier();
    }
    __syncthreads();
    if (threadIdx.x == 0) J.totals[1] = rd(J.B, cell_at(J, 0, 0), 2);
}
#undef FB_RING_THREADS

// A path's summary, as pg_fb_sample and pg_fb_decode_trace write it and the path handles read it, FB_SUMMARY_INTS ints: the status
// (0 a path, 1 full probability zero, 2 internal), the end cell (five ints: state, i, j, k1, k2), the steps, the steps by state,
// a double in two ints (the sampler's log_q, the decoder's objective), four spare
enum { FB_SUM_STATUS = 0, FB_SUM_END = 1, FB_SUM_STEPS = 6, FB_SUM_M = 7, FB_SUM_X = 8, FB_SUM_Y = 9, FB_SUM_VALUE = 10, FB_SUMMARY_INTS = 16 };

#include "dp_fb_deep.inc"
#include "dp_fb_post.inc"
#include "dp_fb_counts.inc"
#include "dp_fb_sample.inc"
#include "dp_fb_decode.inc"

// ---- wide alignments: 64 x 64 blocks on a block-anti-diagonal schedule ----
// Block (a, b) needs blocks (a', b') <= (a, b) only (bwd edges point to earlier sites), so the blocks of one block
// anti-diagonal are independent: workgroup g of the sweep's grid takes the blocks g, g + G, ... of block diagonal t, one
// wave each, and all workgroups meet at a counter barrier before t + 1 -- Lx/64 + Ly/64 barriers per sweep where a barrier
// per cell diagonal cost more than the cells (14 us per diagonal measured: written-through stores, loads from beyond the
// L2).  Inside a block the wave sweeps the block's own 127 anti-diagonals, lane r on row i0 + r: the last FB_RING of them
// live in LDS, and so do the row above / column left of the block (forward) or the row below / column right of it
// (backward); anything else -- an edge that reaches further -- is a load from L2/HBM.  The wave's own stores go out
// unwaited-for; only a read of a cell of its own block that has left the ring waits for them.
// Barrier (MI355X_MICROARCH.md, "Valid forms", producer / consumer with fences): the wave's s_waitcnt vmcnt(0), the
// workgroup barrier, lane 0's agent release + wait, its relaxed agent add; lane 0 polls (relaxed, agent), then agent
// acquire + wait, workgroup barrier, plain loads.
#define FB_RING 12
#define FB_H 8                   // halo depth: rows above / columns left of a block (forward), below / right of it (backward) kept in LDS
#define FB_SPIN_LIMIT (1 << 22)
typedef __attribute__((address_space(1))) int *fb_gi;

struct FbSmem {
    double ring[FB_RING][FB_T][3];
    // forward: ha[u][k] = cell (i0 - FB_H + u, j0 - FB_H + k), the FB_H rows above with the corner; hb[k][u] = cell (i0 + k, j0 - FB_H + u),
    // the FB_H columns to the left.  backward: ha[u][k] = cell (i0 + 64 + u, j0 + k), the rows below with the corner at k >= 64;
    // hb[k][u] = cell (i0 + k, j0 + 64 + u), the columns to the right
    double ha[FB_H][FB_T + FB_H][3];
    double hb[FB_T][FB_H][3];
    // what a step reads besides cells, staged per block: nothing of the common path is a load from memory (a load would
    // queue behind the wave's stores in flight: vector memory operations complete in order)
    int dmin[2 * FB_T], dmax[2 * FB_T];      // band interval of the block's diagonals
    long long doff[2 * FB_T];
    // columns j0 + k: first list entry, entries, the first two entries' other ends and log weights, state (backward: one more column)
    int c_off[FB_T + 1], c_n[FB_T + 1], c_e0[FB_T + 1], c_e1[FB_T + 1], c_st[FB_T + 1];
    float c_lw0[FB_T + 1], c_lw1[FB_T + 1];
    double ltab[256];                // the model's log scores when S * S <= 256
};

// sync[0] arrivals, sync[1] nonzero: a workgroup gave up (a logic error becomes a status instead of a hung GPU).
__device__ __forceinline__ bool fb_barrier(int *sync, int target) {
    __shared__ int ok;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        fb_gi g = (fb_gi)(unsigned long long)sync;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __hip_atomic_fetch_add(g, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        int spins = 0, good = 1;
        while (__hip_atomic_load(g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < target) {
            __builtin_amdgcn_s_sleep(2);
            if ((++spins & 255) == 0 && (spins > FB_SPIN_LIMIT || __hip_atomic_load(g + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0)) {
                __hip_atomic_store(g + 1, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                good = 0;
                break;
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        ok = good;
    }
    __syncthreads();
    return ok != 0;
}

// does block (a, b) hold a cell of the band?
__device__ __forceinline__ bool fb_block_live(const PgFbJob &J, int i0, int j0, int r) {
    bool any = false;
    for (int u = 0; u < 2; ++u) {
        const int d = i0 + j0 + r + 64 * u;
        if (d >= J.nd || r + 64 * u > 2 * FB_T - 2) continue;
        const int lo = max(max(J.imin[d], i0), d - (j0 + FB_T - 1)), hi = min(min(J.imax[d], i0 + FB_T - 1), d - j0);
        any = any || lo <= hi;
    }
    return __builtin_amdgcn_ballot_w64(any) != 0;
}

// The block rows a <= a' <= b that can hold a cell of block anti-diagonal t: the rows of the band's cells on its 127 cell
// diagonals (exact for any band: a minimum and a maximum over the diagonals' intervals).  A tunnel around the main diagonal of
// 2 x 100 kb has 1,563 blocks on its longest block anti-diagonal and a cell in two or three of them.
__device__ __forceinline__ void fb_live_rows(const PgFbJob &J, int t, int r, int &a_first, int &a_last) {
    int lo = 0x7fffffff, hi = -1;
    for (int u = 0; u < 2; ++u) {
        const int d = FB_T * t + r + 64 * u;
        if (d < J.nd && r + 64 * u <= 2 * FB_T - 2) {
            const int mn = J.imin[d], mx = J.imax[d];
            if (mx >= mn) { lo = min(lo, mn); hi = max(hi, mx); }
        }
    }
    for (int w = 32; w >= 1; w >>= 1) { lo = min(lo, __shfl_xor(lo, w, 64)); hi = max(hi, __shfl_xor(hi, w, 64)); }
    a_first = hi < 0 ? 1 : lo / FB_T;
    a_last = hi < 0 ? 0 : hi / FB_T;
}

// lane n takes lane n-1's v; lane 0 keeps `lane0`
__device__ __forceinline__ double fb_shr1(double v, double lane0) {
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __builtin_amdgcn_update_dpp(__double2loint(lane0), lo, 0x138, 0xf, 0xf, false);
    hi = __builtin_amdgcn_update_dpp(__double2hiint(lane0), hi, 0x138, 0xf, 0xf, false);
    return __hiloint2double(hi, lo);
}

// lane n takes lane n+1's v; lane 63 keeps `lane63`
__device__ __forceinline__ double fb_shl1(double v, double lane63) {
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __builtin_amdgcn_update_dpp(__double2loint(lane63), lo, 0x130, 0xf, 0xf, false);
    hi = __builtin_amdgcn_update_dpp(__double2hiint(lane63), hi, 0x130, 0xf, 0xf, false);
    return __hiloint2double(hi, lo);
}

// LDS traffic of the one wave is in order; this keeps the compiler from moving it and waits for nothing in memory
__device__ __forceinline__ void fb_lds_fence() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

__device__ __forceinline__ void fb_stage_diagonals(const PgFbJob &J, FbSmem &M, int dbase, int r) {
    for (int k = r; k < 2 * FB_T; k += 64) {
        const int d = dbase + k;
        const bool in = d < J.nd;
        M.dmin[k] = in ? J.imin[d] : 0; M.dmax[k] = in ? J.imax[d] : -1; M.doff[k] = in ? J.doff[d] : 0;
    }
}

template <bool ALL_LDS>
__global__ __launch_bounds__(64) void pg_fb_forward_tiled(const PgFbJob *jobs) {
    __shared__ FbSmem M;
    const PgFbJob J = jobs[blockIdx.y];
    const int G = J.groups, r = (int)threadIdx.x;
    if ((int)blockIdx.x >= G) return;                              // (a launch is as wide as its widest pair)
    int *sync = J.sync;
    const int nbr = (J.Lx + FB_T - 1) / FB_T, nbc = (J.Ly + FB_T - 1) / FB_T;
    const double NI = ninf();
    const bool tab_lds = J.S * J.S <= 256;
    if (tab_lds) for (int k = r; k < J.S * J.S; k += 64) M.ltab[k] = J.ltab[k];
    for (int t = 0; t < nbr + nbc - 1; ++t) {
        int a_lo = max(0, t - (nbc - 1)), a_hi = min(t, nbr - 1);
        {
            int a_first, a_last;
            fb_live_rows(J, t, r, a_first, a_last);
            a_lo = max(a_lo, a_first); a_hi = min(a_hi, a_last);
        }
        for (int a = a_lo + (int)blockIdx.x; a <= a_hi; a += G) {
            const int i0 = a * FB_T, j0 = (t - a) * FB_T, dbase = i0 + j0;
            if (!fb_block_live(J, i0, j0, r)) continue;
#ifdef PG_FB_STATS
            const unsigned long long st0 = __builtin_readcyclecounter();
#endif
            __syncthreads();                                                       // (the block before is done with the staging arrays)
            // halo: the rows above (with the corner) and the columns to the left; the columns' records; the diagonals' intervals
            for (int k = r; k < FB_H * (FB_T + FB_H); k += 64) {
                const int u = k / (FB_T + FB_H), c_ = k % (FB_T + FB_H);
                const long long at = cell_at(J, i0 - FB_H + u, j0 - FB_H + c_);
                for (int q = 0; q < 3; ++q) M.ha[u][c_][q] = rd(J.F, at, q);
            }
            for (int k = r; k < FB_T * FB_H; k += 64) {
                const int row_ = k / FB_H, u = k % FB_H;
                const long long at = cell_at(J, i0 + row_, j0 - FB_H + u);
                for (int q = 0; q < 3; ++q) M.hb[row_][u][q] = rd(J.F, at, q);
            }
            {
                const int jc = j0 + r;
                const bool cv = jc < J.Ly && jc > 0;
                const int o0 = cv ? J.offR[jc] : 0, o1 = cv ? J.offR[jc + 1] : 0;
                M.c_off[r] = o0; M.c_n[r] = o1 - o0; M.c_st[r] = jc < J.Ly ? J.stR[jc] : 0;
                M.c_e0[r] = o1 > o0 ? J.srcR[o0] : 0; M.c_lw0[r] = o1 > o0 ? J.lwR[o0] : 0.0f;
                M.c_e1[r] = o1 > o0 + 1 ? J.srcR[o0 + 1] : 0; M.c_lw1[r] = o1 > o0 + 1 ? J.lwR[o0 + 1] : 0.0f;
            }
            fb_stage_diagonals(J, M, dbase, r);
            for (int k = r; k < FB_RING * FB_T; k += 64) { double *c = &M.ring[0][0][0] + 3 * k; c[0] = NI; c[1] = NI; c[2] = NI; }
            const int i = i0 + r;
            const bool rv = i < J.Lx && i > 0;
            const int l0 = rv ? J.offL[i] : 0, nl = rv ? J.offL[i + 1] - l0 : 0;
            const int p0 = nl > 0 ? J.srcL[l0] : 0, p1 = nl > 1 ? J.srcL[l0 + 1] : 0, stl = i < J.Lx ? J.stL[i] : 0;
            const double lwl0 = nl > 0 ? (double)J.lwL[l0] : 0.0, lwl1 = nl > 1 ? (double)J.lwL[l0 + 1] : 0.0;
            __syncthreads();
#ifdef PG_FB_STATS
            const unsigned long long st1 = __builtin_readcyclecounter();
#endif
            // The cells a SIMPLE cell reads -- one bwd edge per site, from the previous site -- stay in registers, as in the
            // Viterbi kernels: P this lane's cell of the step before (i, j-1), A the wave shift of P (i-1, j), C the A of the
            // step before (i-1, j-1); a lane starts from the column left of the block, lane 0 takes row i0-1 from the halo.
            const bool row_simple = nl == 1 && p0 == i - 1;
            double Px = M.hb[r][FB_H - 1][0], Py = M.hb[r][FB_H - 1][1], Pm = M.hb[r][FB_H - 1][2];
            double Ax = M.ha[FB_H - 1][FB_H - 1][0], Ay = M.ha[FB_H - 1][FB_H - 1][1], Am = M.ha[FB_H - 1][FB_H - 1][2];   // lane 0: the corner
            double Cx = NI, Cy = NI, Cm = NI;
            for (int s = 0; s <= 2 * FB_T - 2; ++s) {
                const int d = dbase + s;
                if (d >= J.nd) break;
                const int j = d - i, jj = s - r;
                const int mn = M.dmin[s], mx = M.dmax[s];
                const bool active = jj >= 0 && jj < FB_T && i < J.Lx && j < J.Ly && i >= mn && i <= mx;
                double fx = NI, fy = NI, fm = NI;
                {   // this step's register operands
                    const int tc = (s < FB_T ? s : FB_T - 1) + FB_H;               // halo column of (i0-1, j0+s)
                    const double t0 = M.ha[FB_H - 1][tc][0], t1 = M.ha[FB_H - 1][tc][1], t2 = M.ha[FB_H - 1][tc][2];
                    Cx = Ax; Cy = Ay; Cm = Am;
                    Ax = fb_shr1(Px, t0); Ay = fb_shr1(Py, t1); Am = fb_shr1(Pm, t2);
                }
                const bool col_simple = active && M.c_n[jj] == 1 && M.c_e0[jj] == j - 1;
                if (__builtin_amdgcn_ballot_w64(active && !(row_simple && col_simple)) == 0) {
                    if (active) {
                        const double sc = fb_score<ALL_LDS>(tab_lds, M.ltab, J.ltab, stl, M.c_st[jj], J.S);
                        const double w = lwl0 + (double)M.c_lw0[jj];
                        const double mm = J.l_ng + J.l_ng + sc + w, xm = J.l_ng + sc + w;
                        fx = lse3(Ax + J.l_ext, Ay + J.l_open, Am + J.l_ng + J.l_open);                        // VA:2153, 2184, 2215
                        fy = lse3(Py + J.l_ext, Px + J.l_open, Pm + J.l_ng + J.l_open);
                        fm = lse3(Cm + mm, Cx + xm, Cy + xm);                                                  // VA:2051, 2080, 2108
                        const fb_gd o = (fb_gd)(unsigned long long)J.F + 3 * (M.doff[s] + (i - mn));       // (a global store: a flat one counts against lgkmcnt too)
                        o[0] = fx; o[1] = fy; o[2] = fm;
                    }
                } else
                if (active) {
                    auto fetch = [&](int p, int q, double &x, double &y, double &m) {
                        x = NI; y = NI; m = NI;
                        if (p < 0 || q < 0) return;
                        const double *c = nullptr;
                        if (p >= i0 && q >= j0) {
                            if (d - (p + q) < FB_RING) c = M.ring[(p + q) % FB_RING][p - i0];
                            else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // a cell of this block that left the ring: the wave's own store
                        } else if (p < i0 && p >= i0 - FB_H && q >= j0 - FB_H) c = M.ha[p - (i0 - FB_H)][q - (j0 - FB_H)];
                        else if (p >= i0 && q < j0 && q >= j0 - FB_H) c = M.hb[p - i0][q - (j0 - FB_H)];
                        if (c) { x = c[0]; y = c[1]; m = c[2]; return; }
                        const long long at = cell_at(J, p, q);
                        x = rd(J.F, at, 0); y = rd(J.F, at, 1); m = rd(J.F, at, 2);
                    };
                    if (i == 0 && j == 0) {
                        fm = 0.0;                                                  // fwd_score = 1, VA:730
                    } else {
                        double x, y, m;
                        const int r0 = M.c_off[jj], nr = M.c_n[jj], q0 = M.c_e0[jj], q1 = M.c_e1[jj];
                        const double lwr0 = (double)M.c_lw0[jj], lwr1 = (double)M.c_lw1[jj];
                        auto srcl = [&](int k) { return k == 0 ? p0 : (k == 1 ? p1 : J.srcL[l0 + k]); };
                        auto srcr = [&](int k) { return k == 0 ? q0 : (k == 1 ? q1 : J.srcR[r0 + k]); };
                        for (int k = 0; k < nl; ++k) {
                            fetch(srcl(k), j, x, y, m);
                            fx = lse(fx, lse3(x + J.l_ext, y + J.l_open, m + J.l_ng + J.l_open));              // VA:2153, 2184, 2215
                        }
                        for (int k = 0; k < nr; ++k) {
                            fetch(i, srcr(k), x, y, m);
                            fy = lse(fy, lse3(y + J.l_ext, x + J.l_open, m + J.l_ng + J.l_open));
                        }
                        if (nl > 0 && nr > 0) {
                            const double sc = fb_score<ALL_LDS>(tab_lds, M.ltab, J.ltab, stl, M.c_st[jj], J.S);
                            const double mm = J.l_ng + J.l_ng + sc, xm = J.l_ng + sc;                         // VA:1383-1391
                            for (int k1 = 0; k1 < nl; ++k1)
                                for (int k2 = 0; k2 < nr; ++k2) {
                                    fetch(srcl(k1), srcr(k2), x, y, m);
                                    const double w = (k1 == 0 ? lwl0 : (k1 == 1 ? lwl1 : (double)J.lwL[l0 + k1])) +
                                                     (k2 == 0 ? lwr0 : (k2 == 1 ? lwr1 : (double)J.lwR[r0 + k2]));
                                    fm = lse(fm, lse3(m + mm + w, x + xm + w, y + xm + w));                   // VA:2051, 2080, 2108
                                }
                        }
                    }
                    const fb_gd o = (fb_gd)(unsigned long long)J.F + 3 * (M.doff[s] + (i - mn));       // (a global store: a flat one counts against lgkmcnt too)
                    o[0] = fx; o[1] = fy; o[2] = fm;
                }
                double *c = M.ring[d % FB_RING][r];
                c[0] = fx; c[1] = fy; c[2] = fm;
                if (active) { Px = fx; Py = fy; Pm = fm; } else if (jj >= 0) { Px = NI; Py = NI; Pm = NI; }
                fb_lds_fence();
            }
#ifdef PG_FB_STATS
            if (r == 0) {     // sync[16..]: blocks, prologue cycles, step cycles (diagnostic build)
                const unsigned long long st2 = __builtin_readcyclecounter();
                atomicAdd((unsigned long long *)(sync + 16), 1ull); atomicAdd((unsigned long long *)(sync + 18), st1 - st0);
                atomicAdd((unsigned long long *)(sync + 20), st2 - st1);
            }
#endif
        }
#ifdef PG_FB_STATS
        const unsigned long long sb0 = __builtin_readcyclecounter();
#endif
        if (!fb_barrier(sync, G * (t + 1))) return;
#ifdef PG_FB_STATS
        if (r == 0) atomicAdd((unsigned long long *)(sync + 22), __builtin_readcyclecounter() - sb0);
#endif
    }
    if (blockIdx.x == 0 && threadIdx.x == 0)
        J.totals[0] = fb_end_corner(J, [&](int p, int q, int s_) { return rd(J.F, cell_at(J, p, q), s_); });
}

template <bool ALL_LDS>
__global__ __launch_bounds__(64) void pg_fb_backward_tiled(const PgFbJob *jobs) {
    __shared__ FbSmem M;
    const PgFbJob J = jobs[blockIdx.y];
    const int G = J.groups_b, r = (int)threadIdx.x;
    if ((int)blockIdx.x >= G) return;
    int *sync = J.sync + 8;
    const int nbr = (J.Lx + FB_T - 1) / FB_T, nbc = (J.Ly + FB_T - 1) / FB_T;
    const double NI = ninf();
    const bool tab_lds = J.S * J.S <= 256;
    if (tab_lds) for (int k = r; k < J.S * J.S; k += 64) M.ltab[k] = J.ltab[k];
    // (no fill of B: every cell of the band is written by the sweep before anything reads it; what
    //  initialise_array_corner_bwd assigns -- a handful of cells at the end corner, VA:740-854 -- is laid over the -inf a
    //  cell starts from, in the blocks that hold such a cell)
    int round = 0;
    for (int t = nbr + nbc - 2; t >= 0; --t) {
        int a_lo = max(0, t - (nbc - 1)), a_hi = min(t, nbr - 1);
        {
            int a_first, a_last;
            fb_live_rows(J, t, r, a_first, a_last);
            a_lo = max(a_lo, a_first); a_hi = min(a_hi, a_last);
        }
        for (int a = a_lo + (int)blockIdx.x; a <= a_hi; a += G) {
            const int i0 = a * FB_T, j0 = (t - a) * FB_T, dbase = i0 + j0;
            if (!fb_block_live(J, i0, j0, r)) continue;
            __syncthreads();
            // halo: the rows below (with the corner) and the columns to the right; the columns' fwd records (one more column than
            // the block has: a match moves to column j + 1); the diagonals' intervals
            for (int k = r; k < FB_H * (FB_T + FB_H); k += 64) {
                const int u = k / (FB_T + FB_H), c_ = k % (FB_T + FB_H);
                const long long at = cell_at(J, i0 + FB_T + u, j0 + c_);
                for (int q = 0; q < 3; ++q) M.ha[u][c_][q] = rd(J.B, at, q);
            }
            for (int k = r; k < FB_T * FB_H; k += 64) {
                const int row_ = k / FB_H, u = k % FB_H;
                const long long at = cell_at(J, i0 + row_, j0 + FB_T + u);
                for (int q = 0; q < 3; ++q) M.hb[row_][u][q] = rd(J.B, at, q);
            }
            for (int k = r; k <= FB_T; k += 64) {
                const int jc = j0 + k;
                const bool cv = jc < J.Ly;
                const int o0 = cv ? J.foffR[jc] : 0, o1 = cv ? J.foffR[jc + 1] : 0;
                M.c_off[k] = o0; M.c_n[k] = o1 - o0; M.c_st[k] = cv ? J.stR[jc] : 0;
                M.c_e0[k] = o1 > o0 ? J.fdstR[o0] : 0; M.c_lw0[k] = o1 > o0 ? J.flwR[o0] : 0.0f;
                M.c_e1[k] = o1 > o0 + 1 ? J.fdstR[o0 + 1] : 0; M.c_lw1[k] = o1 > o0 + 1 ? J.flwR[o0 + 1] : 0.0f;
            }
            fb_stage_diagonals(J, M, dbase, r);
            for (int k = r; k < FB_RING * FB_T; k += 64) { double *c = &M.ring[0][0][0] + 3 * k; c[0] = NI; c[1] = NI; c[2] = NI; }
            const int i = i0 + r;
            // does an assignment of initialise_array_corner_bwd fall into this block?  (lane r looks at the block's diagonals r, r + 64)
            bool init_here = false;
            for (int u = 0; u < 2 && J.n_init > 0; ++u) {
                const int sd = r + 64 * u, d_ = dbase + sd;
                if (sd > 2 * FB_T - 2 || d_ >= J.nd) continue;
                const int mn_ = J.imin[d_], lo = max(max(mn_, i0), d_ - (j0 + FB_T - 1)), hi = min(min(J.imax[d_], i0 + FB_T - 1), d_ - j0);
                if (lo > hi) continue;
                const long long first = 3 * (J.doff[d_] + (lo - mn_)), last = 3 * (J.doff[d_] + (hi - mn_)) + 2;
                for (int k = 0; k < J.n_init; ++k) init_here = init_here || (J.init_at[k] >= first && J.init_at[k] <= last);
            }
            const bool blk_init = __builtin_amdgcn_ballot_w64(init_here) != 0;
            const bool rv = i < J.Lx;
            const int l0 = rv ? J.foffL[i] : 0, nl = rv ? J.foffL[i + 1] - l0 : 0;
            const int t0 = nl > 0 ? J.fdstL[l0] : 0, t1 = nl > 1 ? J.fdstL[l0 + 1] : 0;
            const int st_t0 = nl > 0 && t0 < J.Lx ? J.stL[t0] : 0, st_t1 = nl > 1 && t1 < J.Lx ? J.stL[t1] : 0;
            const double lwl0 = nl > 0 ? (double)J.flwL[l0] : 0.0, lwl1 = nl > 1 ? (double)J.flwL[l0 + 1] : 0.0;
            __syncthreads();
            // registers, as in the forward sweep but mirrored: P this lane's cell of the step before (i, j+1), A the wave shift
            // that brings lane r+1's P (i+1, j), C the A of the step before (i+1, j+1); a lane starts from the column right of
            // the block, lane 63 takes row i0+64 from the halo
            const bool row_simple = nl == 1 && t0 == i + 1 && t0 < J.Lx;
            double Px = M.hb[r][0][0], Py = M.hb[r][0][1], Pm = M.hb[r][0][2];
            double Ax = M.ha[0][FB_T][0], Ay = M.ha[0][FB_T][1], Am = M.ha[0][FB_T][2];      // lane 63: the corner (i0+64, j0+64)
            double Cx = NI, Cy = NI, Cm = NI;
            for (int s = 2 * FB_T - 2; s >= 0; --s) {
                const int d = dbase + s;
                {   // (every step, also the ones past the matrix's last diagonal: the lanes' columns move with s)
                    const int bc = s - (FB_T - 1);                                   // lane 63's column in the block
                    const int bcc = bc < 0 ? 0 : bc;
                    const double t0_ = M.ha[0][bcc][0], t1_ = M.ha[0][bcc][1], t2_ = M.ha[0][bcc][2];
                    Cx = Ax; Cy = Ay; Cm = Am;
                    (void)Cx; (void)Cy;                                              // (a match moves through M only: VA:2269-2271)
                    Ax = fb_shl1(Px, t0_); Ay = fb_shl1(Py, t1_); Am = fb_shl1(Pm, t2_);
                }
                if (d >= J.nd) continue;
                const int j = d - i, jj = s - r;
                const int mn = M.dmin[s], mx = M.dmax[s];
                const bool active = jj >= 0 && jj < FB_T && i < J.Lx && j < J.Ly && i >= mn && i <= mx;
                double bx = NI, by = NI, bm = NI;
                const bool col_simple = active && M.c_n[jj] == 1 && M.c_e0[jj] == j + 1 && j + 1 < J.Ly;
                if (!blk_init && __builtin_amdgcn_ballot_w64(active && !(row_simple && col_simple)) == 0) {
                    if (active) {
                        const double sc = fb_score<ALL_LDS>(tab_lds, M.ltab, J.ltab, st_t0, M.c_st[jj + 1], J.S);
                        const double thru = Cm + sc + lwl0 + (double)M.c_lw0[jj];             // VA:2269-2271
                        bx = lse3(Ax + J.l_ext, Py + J.l_open, thru + J.l_ng);               // VA:2281-2303
                        by = lse3(Ax + J.l_open, Py + J.l_ext, thru + J.l_ng);
                        bm = lse3(Ax + J.l_ng + J.l_open, Py + J.l_ng + J.l_open, thru + J.l_ng + J.l_ng);
                        const fb_gd o = (fb_gd)(unsigned long long)J.B + 3 * (M.doff[s] + (i - mn));
                        o[0] = bx; o[1] = by; o[2] = bm;
                    }
                } else
                if (active) {
                    // state q of cell (t_, u) >= (i, j)
                    auto fetch = [&](int t_, int u, int q) -> double {
                        if (t_ >= J.Lx || u >= J.Ly) return NI;
                        if (t_ < i0 + FB_T && u < j0 + FB_T) {
                            if ((t_ + u) - d < FB_RING) return M.ring[(t_ + u) % FB_RING][t_ - i0][q];
                            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");       // a cell of this block that left the ring: the wave's own store
                        } else if (t_ >= i0 + FB_T && t_ < i0 + FB_T + FB_H && u < j0 + FB_T + FB_H) return M.ha[t_ - (i0 + FB_T)][u - j0][q];
                        else if (t_ < i0 + FB_T && u >= j0 + FB_T && u < j0 + FB_T + FB_H) return M.hb[t_ - i0][u - (j0 + FB_T)][q];
                        return rd(J.B, cell_at(J, t_, u), q);
                    };
                    const fb_gd o = (fb_gd)(unsigned long long)J.B + 3 * (M.doff[s] + (i - mn));
                    if (blk_init) {
                        const long long at3 = 3 * (M.doff[s] + (i - mn));
                        for (int k = 0; k < J.n_init; ++k) {
                            const long long w = J.init_at[k] - at3;
                            if (w == 0) bx = J.init_val[k]; else if (w == 1) by = J.init_val[k]; else if (w == 2) bm = J.init_val[k];
                        }
                    }
                    const int r0 = M.c_off[jj], nr = M.c_n[jj], u0 = M.c_e0[jj], u1 = M.c_e1[jj];
                    const double lwr0 = (double)M.c_lw0[jj], lwr1 = (double)M.c_lw1[jj];
                    auto dstl = [&](int k) { return k == 0 ? t0 : (k == 1 ? t1 : J.fdstL[l0 + k]); };
                    auto dstr = [&](int k) { return k == 0 ? u0 : (k == 1 ? u1 : J.fdstR[r0 + k]); };
                    for (int k = 0; k < nl; ++k) {                                 // iterate_fwd_edges_for_gap, left site
                        const int t_ = dstl(k);
                        if (t_ >= J.Lx) continue;                                  // VA:1580
                        const double nx = fetch(t_, j, 0);
                        bx = lse(bx, nx + J.l_ext); by = lse(by, nx + J.l_open); bm = lse(bm, nx + J.l_ng + J.l_open);   // VA:2281-2303
                    }
                    for (int k = 0; k < nr; ++k) {
                        const int u = dstr(k);
                        if (u >= J.Ly) continue;
                        const double ny = fetch(i, u, 1);
                        by = lse(by, ny + J.l_ext); bx = lse(bx, ny + J.l_open); bm = lse(bm, ny + J.l_ng + J.l_open);
                    }
                    for (int k1 = 0; k1 < nl; ++k1)                                // iterate_fwd_edges_for_match
                        for (int k2 = 0; k2 < nr; ++k2) {
                            const int t_ = dstl(k1), u = dstr(k2);
                            if (t_ >= J.Lx || u >= J.Ly) continue;
                            const int sl = k1 == 0 ? st_t0 : (k1 == 1 ? st_t1 : J.stL[t_]);
                            const int sr = (u >= j0 && u <= j0 + FB_T) ? M.c_st[u - j0] : J.stR[u];
                            const double sc = fb_score<ALL_LDS>(tab_lds, M.ltab, J.ltab, sl, sr, J.S);
                            const double thru = fetch(t_, u, 2) + sc + (k1 == 0 ? lwl0 : (k1 == 1 ? lwl1 : (double)J.flwL[l0 + k1])) +
                                                (k2 == 0 ? lwr0 : (k2 == 1 ? lwr1 : (double)J.flwR[r0 + k2]));   // VA:2269-2271
                            bx = lse(bx, thru + J.l_ng); by = lse(by, thru + J.l_ng); bm = lse(bm, thru + J.l_ng + J.l_ng);
                        }
                    o[0] = bx; o[1] = by; o[2] = bm;
                }
                double *c = M.ring[d % FB_RING][r];
                c[0] = bx; c[1] = by; c[2] = bm;
                if (active) { Px = bx; Py = by; Pm = bm; } else if (jj < FB_T) { Px = NI; Py = NI; Pm = NI; }
                fb_lds_fence();
            }
        }
        ++round;
        if (!fb_barrier(sync, G * round)) return;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) J.totals[1] = rd(J.B, cell_at(J, 0, 0), 2);
}

} // namespace

int pagan_internal_replay(const pagan_graph *L, const pagan_graph *R, int64_t cells, const int *endcell, double endscore,
                          const int *trace, pagan_result *out);     // dp_abi.hip

// Arenas of finished handles are kept for the next one on the same device (a pair's two matrices are hundreds of MB:
// allocating and freeing them -- a device-wide synchronisation -- per pair was half of a pair's wall-clock); at most 32 (a batch of a tree level's pairs returns that many at once; eight until round 5)
// idle ones per process, pagan_fb_release_cache frees them.
// Idle arenas are bounded by count AND by bytes (a 10 k x 10 k pair's two matrices are 4.8 GB: eight of those idle would
// sit on 38 GB that the Viterbi batches of the same process may need).  A failed allocation frees the idle arenas, which may be
// what is in the way, and tries once more.
namespace {
const SlabPolicy kFbArenaPolicy = {
    /* slack_mul, slack_add */ 2, (size_t)64 << 20, /* grow_div */ 16, /* max_idle */ 32, /* max_idle_per_device */ 0,
    /* max_idle_bytes */ (size_t)8 << 30, /* evict_smallest */ false, /* retry_drained */ true};
SlabPool fb_arena_pool(kFbArenaPolicy);
} // namespace
extern "C" void pagan_fb_internal_release_cache() { drain_slabs(fb_arena_pool, -1); }

struct pagan_fb {
    int device = 0;
    int Lx = 0, Ly = 0, S = 0;
    const pagan_graph *L = nullptr, *R = nullptr;       // borrowed: must outlive the handle for sample_path
    std::vector<float> score;                           // copy of the probability table
    float gap_open = 0, gap_ext = 0, non_gap = 0;
    DiagIndex dx;
    RowBand rb;
    char *arena = nullptr;
    size_t arena_cap = 0;
    size_t arena_bytes = 0;                             // what fb_stage asked of the pool (pagan_fb_device_bytes)
    double *dF = nullptr, *dB = nullptr;
    double totals[2] = {0, 0};
    float kernel_ms[2] = {0, 0};                        // pg_fb_forward, pg_fb_backward (HIP events)
    int groups = 1;                                     // workgroups a diagonal's cells were spread over
    bool ring = false;                                  // the LDS-ring sweeps ran
    bool deep = false;                                  // the deep-ring sweeps (graph pairs) ran
    std::vector<double> hF;                             // downloaded lazily
    PgFbJob job{};                                      // the pair's job record (device pointers into the arena) ...
    const PgFbJob *d_job = nullptr;                     // ... and where it sits on the device
    float post_ms[3] = {0, 0, 0};                       // last pg_fb_gather, row pass, column pass (HIP events)
    float counts_ms = 0;                                // last pg_fb_counts + pg_fb_counts_fold (booked at a batch's first pair)
    long long at(int i, int j) const { return dx.at(i, j); }
};

namespace {
// The arena's arrays, each named once: add() reserves the array's range (rounded up to 256 bytes) and remembers where its bytes
// come from and which pointer of the job record is to point at it; bind() fills the staging buffer and sets the pointers once
// the arena's base is known.
struct FbLayout {
    struct Item { size_t off, bytes; const void *src; void *field; };
    std::vector<Item> items;
    size_t cur = 0;
    template <class P>
    void add(const void *src, size_t bytes, P **field) {
        items.push_back({cur, bytes, src, (void *)field});
        cur = (cur + bytes + 255) / 256 * 256;
    }
    void bind(char *base, char *stage) const {
        for (const Item &it : items) { char *p = base + it.off; std::memcpy(it.field, &p, sizeof(p)); }
        for (const Item &it : items) if (it.src && it.bytes) std::memcpy(stage + it.off, it.src, it.bytes);
    }
};

// One call that reads finished passes of one device: the thread on that device for the call's length, one device buffer laid
// out by take() -- first what goes UP (job records, launch records, small inputs), then what comes DOWN with the call (results,
// summaries), then what only the DEVICE sees (partial sums, traces, pack buffers), every piece rounded up to 256 bytes --, the
// host's copy of the first two regions, and the launches' times: begin() / end() around the launches of a span, any number of
// spans, ms(k) once download() has waited for them.  The buffer is shared so that the handles a call makes can keep it.
struct FbCall {
    enum Region { UP, DOWN, DEVICE };
    std::optional<DeviceScope> on_device;
    std::shared_ptr<DevBuf> buf = std::make_shared<DevBuf>();
    std::vector<char> host;
    std::vector<Event> ev;                 // a span's two events
    size_t cur = 0, end_of[3] = {0, 0, 0};
    int open(int32_t n, pagan_fb *const *fbs) {
        for (int k = 0; k < n; ++k) if (!fbs[k] || fbs[k]->device != fbs[0]->device) return PAGAN_E_ARG;
        on_device.emplace(fbs[0]->device);
        return on_device->ok ? PAGAN_OK : PAGAN_E_NODEVICE;
    }
    size_t take(Region r, size_t bytes) {
        const size_t at = cur;
        cur = up256(cur + bytes);
        for (int q = r; q < 3; ++q) end_of[q] = cur;
        return at;
    }
    int alloc() { host.assign(end_of[DOWN], 0); FB_TRY(buf->alloc(cur)); return PAGAN_OK; }
    template <class T> T *dev(size_t off) const { return (T *)(buf->h + off); }
    template <class T> void put(size_t off, const T &rec) { std::memcpy(host.data() + off, &rec, sizeof(T)); }
    int upload() { FB_TRY(hipMemcpy(buf->h, host.data(), end_of[UP], hipMemcpyHostToDevice)); return PAGAN_OK; }
    int begin() {
        for (int q = 0; q < 2; ++q) { ev.emplace_back(); FB_TRY(ev.back().create()); }
        FB_TRY(hipEventRecord(ev[ev.size() - 2], nullptr));
        return PAGAN_OK;
    }
    int end() { FB_TRY(hipGetLastError()); FB_TRY(hipEventRecord(ev.back(), nullptr)); return PAGAN_OK; }
    int download() {
        FB_TRY(hipMemcpy(host.data() + end_of[UP], buf->h + end_of[UP], end_of[DOWN] - end_of[UP], hipMemcpyDeviceToHost));
        return PAGAN_OK;
    }
    float ms(int span) const { float v = 0; (void)hipEventElapsedTime(&v, ev[2 * span], ev[2 * span + 1]); return v; }
};

// One planned pair up to the upload of its inputs: the arena, the job record with its workgroup count
// (`groups_cap`, `groups_cap_b`: what the caller's launch leaves this pair's forward / backward sweep).  Nothing is decided here:
// the schedule, the workgroup and every array but the score table come with the plan, whose band index the handle keeps.
struct FbStaged {
    std::unique_ptr<pagan_fb, void (*)(pagan_fb *)> fb{nullptr, pagan_fb_destroy};
    int groups_b = 1;                        // workgroups of the backward tiled sweep (the forward sweep's: fb->groups)
    int block = 64, nsplit = 1;              // FbPlan's
    double t_host[3] = {0, 0, 0};            // band index + lists, arena, upload (seconds)
    size_t arena_bytes = 0;
};
static double fb_now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
// what fb_plan_pair does not look at, in the order the errors have always come in: the arguments, the graphs, the model, a device
static int fb_check_pair(const pagan_graph *left, const pagan_graph *right, const pagan_model_prob *model) {
    if (!left || !right || !model || !model->score || model->n_states < 1) return PAGAN_E_ARG;
    int rc = check_graph(left);
    if (rc == PAGAN_OK) rc = check_graph(right);
    if (rc != PAGAN_OK) return rc;
    const int S = model->n_states;
    for (int s = 1; s < left->n_sites - 1; ++s) if (left->state[s] < 0 || left->state[s] >= S) return PAGAN_E_MODEL;
    for (int s = 1; s < right->n_sites - 1; ++s) if (right->state[s] < 0 || right->state[s] >= S) return PAGAN_E_MODEL;
    if (!(model->gap_open > 0) || !(model->gap_ext > 0) || !(model->non_gap > 0)) return PAGAN_E_MODEL;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return PAGAN_E_NODEVICE;
    return PAGAN_OK;
}
static int fb_stage(FbPlan &plan, const pagan_graph *left, const pagan_graph *right, const pagan_model_prob *model,
                    const pagan_opts *opts, int groups_cap, int groups_cap_b, FbStaged *st) {
    const int Lx = plan.Lx, Ly = plan.Ly, S = model->n_states;
    const double th0 = fb_now();
    st->fb.reset(new pagan_fb());            // (st owns the handle: an error from here on destroys it with st)
    pagan_fb *fb = st->fb.get();
    if (opts && opts->device >= 0) { FB_TRY(hipSetDevice(opts->device)); fb->device = opts->device; }
    else FB_TRY(hipGetDevice(&fb->device));
    fb->Lx = Lx; fb->Ly = Ly; fb->S = S; fb->L = left; fb->R = right;
    fb->score.assign(model->score, model->score + (size_t)S * S);
    fb->gap_open = model->gap_open; fb->gap_ext = model->gap_ext; fb->non_gap = model->non_gap;
    fb->rb = std::move(plan.rb); fb->dx = std::move(plan.dx);
    const long long cells = fb->dx.cells;
    std::vector<double> ltab((size_t)S * S);
    for (size_t k = 0; k < ltab.size(); ++k) ltab[k] = std::log((double)model->score[k]);
    fb->groups = plan.groups_within(groups_cap); st->groups_b = plan.groups_within(groups_cap_b);
    fb->ring = plan.ring; fb->deep = plan.deep;
    st->block = plan.block; st->nsplit = plan.nsplit;
    PgFbJob &J = fb->job;
    J.Lx = Lx; J.Ly = Ly; J.nd = plan.nd; J.S = S;
    J.l_ext = std::log((double)model->gap_ext); J.l_open = std::log((double)model->gap_open); J.l_ng = std::log((double)model->non_gap);
    J.cells = cells;
    J.n_init = (int)plan.init_at.size(); J.init_dmin = plan.init_dmin;
    J.groups = fb->groups; J.groups_b = st->groups_b;
    J.nseg = (int)plan.seg_B.size();
    // one arena: the job record and the inputs, then F and B (pagan_fb_predict_bytes and the pool's fit rule know this layout)
    FbLayout lay;
    auto vec = [&](const auto &v, auto **field) { lay.add(v.data(), sizeof(v[0]) * v.size(), field); };
    const size_t nL = (size_t)left->n_sites, nR = (size_t)right->n_sites, nbL = (size_t)left->bwd_off[nL], nbR = (size_t)right->bwd_off[nR];
    lay.add(&J, sizeof(PgFbJob), &fb->d_job);
    lay.add(left->state, 4 * nL, &J.stL); lay.add(left->bwd_off, 4 * (nL + 1), &J.offL); lay.add(left->bwd_src, 4 * nbL, &J.srcL); lay.add(left->bwd_logw, 4 * nbL, &J.lwL);
    lay.add(right->state, 4 * nR, &J.stR); lay.add(right->bwd_off, 4 * (nR + 1), &J.offR); lay.add(right->bwd_src, 4 * nbR, &J.srcR); lay.add(right->bwd_logw, 4 * nbR, &J.lwR);
    vec(plan.fl.off, &J.foffL); vec(plan.fl.dst, &J.fdstL); vec(plan.fl.lw, &J.flwL);
    vec(plan.fr.off, &J.foffR); vec(plan.fr.dst, &J.fdstR); vec(plan.fr.lw, &J.flwR);
    vec(ltab, &J.ltab);
    vec(fb->dx.imin, &J.imin); vec(fb->dx.imax, &J.imax); vec(fb->dx.doff, &J.doff);
    vec(plan.init_at, &J.init_at); vec(plan.init_val, &J.init_val);
    vec(plan.seg_start, &J.seg_start); vec(plan.seg_B, &J.seg_B); vec(plan.dfar, &J.dfar);
    lay.add(nullptr, 16, &J.totals);
    lay.add(nullptr, 256, &J.sync);                       // two barrier counters + give-up words of the wide sweeps (zero)
    const size_t in_bytes = lay.cur;
    lay.add(nullptr, 24 * (size_t)cells, &J.F); lay.add(nullptr, 24 * (size_t)cells, &J.B);
    const double th1 = fb_now();
    fb->arena = slab_alloc(fb_arena_pool, fb->device, lay.cur, &fb->arena_cap);
    if (!fb->arena) return PAGAN_E_NOMEM;
    std::vector<char> stage(in_bytes, 0);
    lay.bind(fb->arena, stage.data());
    fb->dF = J.F; fb->dB = J.B;
    const double th2 = fb_now();
    FB_TRY(hipMemcpy(fb->arena, stage.data(), in_bytes, hipMemcpyHostToDevice));
    st->t_host[0] += th1 - th0; st->t_host[1] = th2 - th1; st->t_host[2] = fb_now() - th2;
    st->arena_bytes = fb->arena_bytes = lay.cur;
    return PAGAN_OK;
}

// ... and behind the kernels: the kernel times, the totals, the barriers' give-up words
static int fb_finish(FbStaged *st, float fwd_ms, float bwd_ms) {
    pagan_fb *fb = st->fb.get();
    fb->kernel_ms[0] = fwd_ms; fb->kernel_ms[1] = bwd_ms;
    FB_TRY(hipMemcpy(fb->totals, fb->job.totals, 16, hipMemcpyDeviceToHost));
    int sy[64];
    FB_TRY(hipMemcpy(sy, fb->job.sync, sizeof(sy), hipMemcpyDeviceToHost));
    if (sy[1] != 0 || sy[9] != 0) return PAGAN_E_INTERNAL;          // a barrier of a wide sweep ran into its limit
#ifdef PG_FB_STATS
    {
        const unsigned long long *q = (const unsigned long long *)(sy + 16);
        std::fprintf(stderr, "pagan_fb: forward: %llu blocks, prologue %.0f cycles per block, steps %.0f per block, barrier %.0f per workgroup and block diagonal (%d groups)\n",
                     q[0], q[0] ? (double)q[1] / q[0] : 0.0, q[0] ? (double)q[2] / q[0] : 0.0,
                     (double)q[3] / fb->groups / ((fb->Lx + 63) / 64 + (fb->Ly + 63) / 64 - 1), fb->groups);
    }
#endif
    return PAGAN_OK;
}

// A sweep whose workgroups meet at a counter barrier needs ALL of them on the chip at once; a caller may have any number
// of alignments in flight from as many threads, and workgroups of one sweep holding compute units while they wait for
// siblings that other waiting sweeps keep out would never end (the barrier's spin limit would turn that into an error,
// seconds later).  So the tiled sweeps of a device share a budget of workgroup slots well inside what the device holds
// at this kernel's LDS size (3 per compute unit); a launch that does not fit waits here, on the host.
struct FbSlots {
    std::mutex m; std::condition_variable cv; int used = 0;
    void take(int n, int cap) { std::unique_lock<std::mutex> l(m); cv.wait(l, [&] { return used == 0 || used + n <= cap; }); used += n; }
    void give(int n) { { std::lock_guard<std::mutex> l(m); used -= n; } cv.notify_all(); }
};
static FbSlots fb_slots_of[64];
struct FbSlotLease { FbSlots *s; int n; ~FbSlotLease() { if (n > 0) s->give(n); } };
static int fb_slot_cap(int device, const FbSwitches &sw) {
    int n_cu = 0;
    if (hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && n_cu > 0) return sw.slots_x16 * n_cu / 16;
    return 512;
}

// The four schedules' kernels behind one launch.  `block`: the threads of a one-workgroup, tiled or deep-ring workgroup, the rows
// B of a ring sweep's -- its workgroup has `nsplit` threads a row: three up to B = 256, two with 512 (PAGAN_FB_RING_SPLIT=0: one), see
// FB_RING_THREADS; 1,024 threads is what a workgroup holds.  all_lds: every pair's score table fits LDS (the kernels without the
// table's load from memory; the one-workgroup kernels have one form).
enum FbKind { FB_K_SMALL = 0, FB_K_TILED = 1, FB_K_RING = 2, FB_K_DEEP = 3 };      // (pagan_fb_schedule's codes)
typedef void (*FbKernel)(const PgFbJob *);
template <bool ALL_LDS>
static FbKernel fb_kernel(FbKind kind, bool fwd, int block, int nsplit) {
    if (kind == FB_K_TILED) return fwd ? pg_fb_forward_tiled<ALL_LDS> : pg_fb_backward_tiled<ALL_LDS>;
    if (kind == FB_K_DEEP) return fwd ? pg_fb_forward_deep<ALL_LDS> : pg_fb_backward_deep<ALL_LDS>;
    if (kind == FB_K_SMALL) return fwd ? pg_fb_forward : pg_fb_backward;
    if (block > 512) return fwd ? pg_fb_forward_ring<ALL_LDS, 1, 1024> : pg_fb_backward_ring<ALL_LDS, 1, 1024>;
    if (nsplit == 3) return fwd ? pg_fb_forward_ring<ALL_LDS, 3, 512> : pg_fb_backward_ring<ALL_LDS, 3, 512>;
    if (nsplit == 2) return fwd ? pg_fb_forward_ring<ALL_LDS, 2, 512> : pg_fb_backward_ring<ALL_LDS, 2, 512>;
    return fwd ? pg_fb_forward_ring<ALL_LDS, 1, 512> : pg_fb_backward_ring<ALL_LDS, 1, 512>;
}
static void fb_launch(FbKind kind, bool fwd, bool all_lds, dim3 grid, int block, int nsplit, hipStream_t stream, const PgFbJob *jobs) {
    const FbKernel k = all_lds ? fb_kernel<true>(kind, fwd, block, nsplit) : fb_kernel<false>(kind, fwd, block, nsplit);
    hipLaunchKernelGGL(k, grid, dim3((unsigned)(nsplit * block)), 0, stream, jobs);
}

// A chunk's launches are described before any goes out.  A GROUP is one launch per direction: the pairs that share a kind, a
// workgroup size and `all_lds`.  A SPAN is what is timed as one: the groups [a, z) of one kind, side by side -- the first on
// the span's two streams (forward, backward), each other on streams of its own that those two wait for, so that the events
// around the two span them all.  The tiled pairs are one group; the ring pairs one span, the deep-ring pairs another, of a group
// per (workgroup size, table in LDS or not) -- a handful at most; a one-workgroup pair is a group and a span of its own.
// (Only the tiled group is charged to the slot budget: see ADVICE.md's fourth finding; this list is where the others would be.)
struct FbGroup {
    FbKind kind; bool all_lds; int block, nsplit;
    unsigned gx, gx_b, gy;                   // the grid: x of the forward / of the backward launch, y
    std::vector<int> ks;                     // its pairs, in the order of its job records
    const PgFbJob *jobs;                     // ... which are here on the device
};
struct FbSpan {
    size_t a, z; bool timed;
    hipStream_t lane[2]; hipEvent_t ev[4];   // forward, backward; forward's start and end, backward's
};
// what a chunk's launches run on (the streams last: they are synchronised and destroyed before anything else goes)
struct FbChunkRes {
    std::vector<Event> events;
    std::vector<Stream> streams;
    int stream(hipStream_t *s) { streams.emplace_back(); FB_TRY(streams.back().create()); *s = streams.back(); return PAGAN_OK; }
    int event(bool timing, hipEvent_t *e) { events.emplace_back(); FB_TRY(events.back().create(timing)); *e = events.back(); return PAGAN_OK; }
};
static int fb_launch_span(FbChunkRes &res, const std::vector<FbGroup> &groups, FbSpan &S, bool bwd_first) {
    for (int dir = 0; dir < 2; ++dir) FB_DO(res.stream(&S.lane[dir]));
    for (int q = 0; q < 4 && S.timed; ++q) FB_DO(res.event(true, &S.ev[q]));
    for (size_t g = S.a; g < S.z; ++g) {
        const FbGroup &G = groups[g];
        for (int q = 0; q < 2; ++q) {
            const int dir = bwd_first ? 1 - q : q;
            hipStream_t s = S.lane[dir];
            if (g > S.a) FB_DO(res.stream(&s));
            else if (S.timed) FB_TRY(hipEventRecord(S.ev[2 * dir], s));
            fb_launch(G.kind, dir == 0, G.all_lds, dim3(dir ? G.gx_b : G.gx, G.gy), G.block, G.nsplit, s, G.jobs);
            if (g > S.a) {
                hipEvent_t done = nullptr;
                FB_DO(res.event(false, &done));
                FB_TRY(hipEventRecord(done, s)); FB_TRY(hipStreamWaitEvent(S.lane[dir], done, 0));
            }
        }
    }
    if (S.timed) { FB_TRY(hipEventRecord(S.ev[1], S.lane[0])); FB_TRY(hipEventRecord(S.ev[3], S.lane[1])); }
    return PAGAN_OK;
}

// A chunk of pairs whose tiled sweeps fit the slot budget: staged, launched, synchronised, their totals fetched.  st[q].fb is the
// caller's to hand back or to destroy -- after this function has returned, that is after every stream of the chunk has been
// synchronised by its owner, whichever way the function was left.  `only_pair`: the chunk is the call's one pair.
static int fb_run_chunk(int chunk, const pagan_graph *const *left, const pagan_graph *const *right, const pagan_model_prob *const *model,
                        const pagan_band *const *band, const pagan_opts *opts, bool only_pair, int cap, const FbSwitches &sw, FbStaged *st) {
    const int device = opts->device;
    // the backward sweep is the slower of the two when a block anti-diagonal takes several turns: it gets the larger share
    // of the slots (PAGAN_FB_SPLIT: the forward sweeps' per cent, A/B).  A single pair's caps come out at or above FB_MAX_GROUPS
    // at the default budget; with PAGAN_FB_SLOTS_X16 near its minimum they can cut a single pair's sweeps too.
    const int per_pair = std::max(4, cap / chunk);            // slots of one pair, both sweeps
    const int groups_cap = std::max(2, (per_pair * sw.split + 50) / 100), groups_cap_b = std::max(2, per_pair - groups_cap);
    std::vector<int> rcs(chunk, PAGAN_OK);
    auto stage = [&](int q) {
        if ((rcs[q] = fb_check_pair(left[q], right[q], model[q])) != PAGAN_OK) return;
        const double t0 = fb_now();
        FbPlan plan;
        if ((rcs[q] = fb_plan_pair(left[q], right[q], band ? band[q] : nullptr, sw, &plan, std::log((double)model[q]->non_gap))) != PAGAN_OK) return;
        st[q].t_host[0] = fb_now() - t0;
        rcs[q] = fb_stage(plan, left[q], right[q], model[q], opts, groups_cap, groups_cap_b, &st[q]);
    };
    if (chunk == 1) stage(0);        // on the calling thread: a caller with a thread per pair makes no second thread per call
    else {
        std::vector<std::thread> pool;
        std::atomic<int> next{0};
        for (int t = 0; t < std::min(chunk, 16); ++t) pool.emplace_back([&] {
            const bool on = hipSetDevice(device) == hipSuccess;
            for (int q; (q = next.fetch_add(1)) < chunk;) { if (on) stage(q); else rcs[q] = PAGAN_E_NODEVICE; }
        });
        for (auto &th : pool) th.join();
    }
    int rc = PAGAN_OK;
    for (int q = 0; q < chunk; ++q) if (rcs[q] != PAGAN_OK) rc = rcs[q];
    if (rc != PAGAN_OK) return rc;
    for (int q = 0; q < chunk; ++q) if (st[q].fb->device != device) return PAGAN_E_INTERNAL;      // (every pair's arena is on the launches' device)
    const double th3 = fb_now();
    // the launch groups, in the order they go out: tiled, ring, one-workgroup, and the deep-ring groups last (below)
    auto lds = [&](int q) { return fb_table_in_lds(st[q].fb->S); };
    auto key = [&](int q) { return 2 * st[q].block + (lds(q) ? 1 : 0); };              // workgroup size, table in LDS
    std::vector<int> of[4];
    for (int q = 0; q < chunk; ++q) of[st[q].fb->groups > 1 ? FB_K_TILED : (st[q].fb->deep ? FB_K_DEEP : (st[q].fb->ring ? FB_K_RING : FB_K_SMALL))].push_back(q);
    std::vector<FbGroup> groups;
    std::vector<FbSpan> spans;
    std::vector<PgFbJob> jobs;           // the records of the groups of several pairs, group by group
    int slots_needed = 0;
    for (FbKind kind : {FB_K_TILED, FB_K_RING, FB_K_SMALL, FB_K_DEEP}) {
        std::vector<int> &ks = of[kind];
        if (kind == FB_K_RING || kind == FB_K_DEEP) std::stable_sort(ks.begin(), ks.end(), [&](int a, int b) { return key(a) < key(b); });
        for (size_t a = 0, z; a < ks.size(); a = z) {
            z = kind == FB_K_TILED ? ks.size() : a + 1;
            while (kind != FB_K_SMALL && z < ks.size() && key(ks[z]) == key(ks[a])) ++z;
            FbGroup G{kind, true, st[ks[a]].block, st[ks[a]].nsplit, (unsigned)(z - a), (unsigned)(z - a), 1, {ks.begin() + a, ks.begin() + z}, st[ks[a]].fb->d_job};
            if (kind == FB_K_TILED) { G.gx = G.gx_b = 0; G.gy = (unsigned)(z - a); }
            for (int q : G.ks) {
                G.all_lds = G.all_lds && lds(q);
                if (kind != FB_K_TILED) continue;
                G.gx = std::max(G.gx, (unsigned)st[q].fb->groups); G.gx_b = std::max(G.gx_b, (unsigned)st[q].groups_b);   // (a launch is as wide as its widest pair)
                slots_needed += st[q].fb->groups + st[q].groups_b;
            }
            // (a group of one pair launches on the record in the pair's own arena; the others' records: one array, one copy, below)
            if (G.ks.size() > 1) { G.jobs = nullptr; for (int q : G.ks) jobs.push_back(st[q].fb->job); }
            if (a == 0 || kind == FB_K_SMALL) spans.push_back({groups.size(), groups.size(), kind != FB_K_SMALL || only_pair, {nullptr, nullptr}, {nullptr, nullptr, nullptr, nullptr}});
            spans.back().z = groups.size() + 1;
            groups.push_back(std::move(G));
        }
    }
    // Owners, in the order they must outlive each other: the records, the slot lease, the events, the streams.
    DevBuf d_jobs;
    FbSlotLease lease{&fb_slots_of[device & 63], 0};
    FbChunkRes res;
    if (!jobs.empty()) {
        FB_TRY(d_jobs.alloc(jobs.size() * sizeof(PgFbJob)));
        FB_TRY(hipMemcpy(d_jobs, jobs.data(), jobs.size() * sizeof(PgFbJob), hipMemcpyHostToDevice));
        const PgFbJob *at = (const PgFbJob *)d_jobs.h;
        for (FbGroup &G : groups) if (!G.jobs) { G.jobs = at; at += G.ks.size(); }
    }
    // the lease is taken before the tiled launches and given back at the end of the chunk
    if (slots_needed > 0) { lease.s->take(slots_needed, cap); lease.n = slots_needed; }
    for (FbSpan &S : spans) {
        const FbKind kind = groups[S.a].kind;
        if (kind == FB_K_DEEP) {
            // behind the tiled sweeps: a deep-ring workgroup declares 153 KB of LDS, so no tiled workgroup shares its compute unit, and
            // the tiled sweeps' slot budget counts on three a compute unit being resident at once -- the deep launches go out once the
            // tiled streams are synchronised
            FB_TRY(hipGetLastError());
            if (groups[0].kind == FB_K_TILED) { FB_TRY(hipStreamSynchronize(spans[0].lane[0])); FB_TRY(hipStreamSynchronize(spans[0].lane[1])); }
        }
        FB_DO(fb_launch_span(res, groups, S, sw.bwd_first && kind == FB_K_TILED));      // (A/B: which tiled sweep's workgroups are dealt out first)
    }
    FB_TRY(hipGetLastError());
    const double th4 = fb_now();
    for (const Stream &s : res.streams) FB_TRY(hipStreamSynchronize(s));
    const double th5 = fb_now();
    // A span's two times go to its first pair, 0 to its others: a sum over the batch is the launches'.  (A one-workgroup pair is
    // timed when it is the call's only pair.)
    for (const FbSpan &S : spans) {
        float ms[2] = {0, 0};
        if (S.timed) { (void)hipEventElapsedTime(&ms[0], S.ev[0], S.ev[1]); (void)hipEventElapsedTime(&ms[1], S.ev[2], S.ev[3]); }
        for (size_t g = S.a; g < S.z; ++g)
            for (int q : groups[g].ks) {
                const bool first = q == groups[S.a].ks[0];
                FB_DO(fb_finish(&st[q], first ? ms[0] : 0.0f, first ? ms[1] : 0.0f));
            }
    }
    if (sw.verbose) {
        double t[3] = {0, 0, 0}, mb = 0;
        for (int q = 0; q < chunk; ++q) { for (int k = 0; k < 3; ++k) t[k] += st[q].t_host[k]; mb += st[q].arena_bytes / 1048576.0; }
        std::fprintf(stderr, "pagan_fb: host: %d pair(s): band index + lists %.1f ms, arena (%.0f MB) %.1f ms, upload %.1f ms, streams + launch (+ slot wait) %.1f ms, kernels %.1f ms, rest %.1f ms\n",
                     chunk, 1e3 * t[0], mb, 1e3 * t[1], 1e3 * t[2], 1e3 * (th4 - th3), 1e3 * (th5 - th4), 1e3 * (fb_now() - th5));
    }
    return PAGAN_OK;
}

} // namespace

extern "C" {

// Several pairs at once (round 5): the sweeps of ALL the pairs' wide matrices in ONE launch per direction, grid = (most workgroups
// of any pair, pairs) -- concurrency is no longer what the HIP runtime's hardware queues allow (eight kernels at a time: four
// pairs), but what the chip holds.  Every tiled pair gets an equal share of the device's workgroup slots (its sweeps may then
// take a block anti-diagonal in two or three turns); pairs whose diagonals are narrow keep their one-workgroup kernels, a
// stream per direction each.  On an error nothing is handed back and every staged handle is destroyed.
int pagan_fb_run_batch(int32_t n, const pagan_graph *const *left, const pagan_graph *const *right, const pagan_model_prob *const *model,
                       const pagan_band *const *band, const pagan_opts *opts, pagan_fb **out) {
    if (n < 0 || (n > 0 && (!left || !right || !model || !out))) return PAGAN_E_ARG;
    for (int k = 0; k < n; ++k) out[k] = nullptr;
    for (int k = 0; k < n; ++k) if (!left[k] || !right[k] || !model[k]) return PAGAN_E_ARG;
    if (n == 0) return PAGAN_OK;
    // the device, resolved once: the calling thread is put on it before any allocation, stream or launch (a caller may pass a
    // device that is not its current one), the staging threads are handed it, and the caller's device is restored on the way out
    DeviceScope on_device(opts ? opts->device : -1);
    if (!on_device.ok) return PAGAN_E_NODEVICE;
    pagan_opts staged_opts;
    staged_opts.flags = opts ? opts->flags : 0u;
    staged_opts.device = on_device.device;
    const FbSwitches sw = FbSwitches::read();
    const int cap = fb_slot_cap(staged_opts.device, sw);
    std::vector<FbStaged> st(n);         // owns the handles until they are handed back
    // chunks of pairs whose tiled sweeps fit the slot budget with at least eight workgroups a sweep
    for (int done = 0, chunk; done < n; done += chunk) {
        chunk = std::min(n - done, std::max(1, cap / 16));
        FB_DO(fb_run_chunk(chunk, left + done, right + done, model + done, band ? band + done : nullptr, &staged_opts, n == 1, cap, sw, &st[done]));
    }
    for (int k = 0; k < n; ++k) out[k] = st[k].fb.release();
    return PAGAN_OK;
}

// One pair: the batch of one.  Like every other entry point it leaves the calling thread on the device it came with (until the two
// calls shared one path, this one left the thread on opts->device).
int pagan_fb_run(const pagan_graph *left, const pagan_graph *right, const pagan_model_prob *model, const pagan_band *band,
                 const pagan_opts *opts, pagan_fb **out) {
    if (!out) return PAGAN_E_ARG;
    return pagan_fb_run_batch(1, &left, &right, &model, band ? &band : nullptr, opts, out);
}

int pagan_fb_kernel_ms(const pagan_fb *fb, double ms[2]) {
    if (!fb || !ms) return PAGAN_E_ARG;
    ms[0] = fb->kernel_ms[0]; ms[1] = fb->kernel_ms[1];
    return PAGAN_OK;
}

int pagan_fb_device_bytes(const pagan_fb *fb, int64_t *bytes) {
    if (!fb || !bytes) return PAGAN_E_ARG;
    *bytes = (int64_t)fb->arena_bytes;
    return PAGAN_OK;
}

int pagan_fb_groups(const pagan_fb *fb) { return fb ? (fb->ring || fb->deep ? 0 : fb->groups) : PAGAN_E_ARG; }

int pagan_fb_schedule(const pagan_fb *fb) { return fb ? (fb->deep ? 3 : (fb->ring ? 2 : (fb->groups > 1 ? 1 : 0))) : PAGAN_E_ARG; }

int pagan_fb_totals(const pagan_fb *fb, double *log_fwd, double *log_bwd, int64_t *cells) {
    if (!fb) return PAGAN_E_ARG;
    if (log_fwd) *log_fwd = fb->totals[0];
    if (log_bwd) *log_bwd = fb->totals[1];
    if (cells) *cells = fb->dx.cells;
    return PAGAN_OK;
}

// which: 0 = log forward, 1 = log backward, 2 = posterior (compute_posterior_score, VA:1029-1034).
// dst [Lx][Ly][3] row-major, state order X, Y, M; outside the tunnel -inf (logs) / 0 (posterior).
int pagan_fb_dump(pagan_fb *fb, int32_t which, double *dst) {
    if (!fb || !dst || which < 0 || which > 2) return PAGAN_E_ARG;
    DeviceScope on_device(fb->device);
    if (!on_device.ok) return PAGAN_E_NODEVICE;
    const size_t n = 3 * (size_t)fb->dx.cells;
    std::vector<double> a(n), bb;
    FB_TRY(hipMemcpy(a.data(), which == 1 ? fb->dB : fb->dF, 8 * n, hipMemcpyDeviceToHost));
    if (which == 2) { bb.resize(n); FB_TRY(hipMemcpy(bb.data(), fb->dB, 8 * n, hipMemcpyDeviceToHost)); }
    const double outside = which == 2 ? 0.0 : -HUGE_VAL;
    for (int i = 0; i < fb->Lx; ++i)
        for (int j = 0; j < fb->Ly; ++j) {
            const long long at = fb->at(i, j);
            double *o = dst + ((size_t)i * fb->Ly + j) * 3;
            for (int s = 0; s < 3; ++s) {
                if (at < 0) { o[s] = outside; continue; }
                if (which != 2) { o[s] = a[3 * at + s]; continue; }
                // fb_post's zero rule (dp_fb_post.inc): a pair whose full probability is 0 has posterior 0 in every cell -- the
                // argument is then -inf minus -inf, a NaN, which compares false.  Its clamp of the argument to <= 0 is NOT taken over:
                // as before, a value here may exceed 1 by an ulp where pg_fb_gather returns exactly 1
                const double x = a[3 * at + s] + bb[3 * at + s] - fb->totals[0];
                o[s] = x > -HUGE_VAL ? std::exp(x) : 0.0;
            }
        }
    return PAGAN_OK;
}

} // extern "C"

namespace {
// pg_fb_gather over one pair: the triples go up in one copy, the posteriors come back in one (state outside 0..2: -1)
static int fb_gather(pagan_fb *fb, int32_t n, const int32_t *cells, double *post) {
    if (n == 0) return PAGAN_OK;
    FbCall c;
    FB_DO(c.open(1, &fb));
    const size_t o_rec = c.take(FbCall::UP, sizeof(PgFbGather)), o_cells = c.take(FbCall::UP, 12 * (size_t)n);
    const size_t o_out = c.take(FbCall::DOWN, 8 * (size_t)n);
    FB_DO(c.alloc());
    PgFbGather G;
    G.cells = c.dev<const int>(o_cells); G.out = c.dev<double>(o_out); G.n = n;
    c.put(o_rec, G);
    std::memcpy(c.host.data() + o_cells, cells, 12 * (size_t)n);
    FB_DO(c.upload());
    FB_DO(c.begin());
    const unsigned blocks = (unsigned)std::min<long long>(((long long)n + 255) / 256, 4096);
    hipLaunchKernelGGL(pg_fb_gather, dim3(blocks, 1), dim3(256), 0, nullptr, fb->d_job, c.dev<const PgFbGather>(o_rec));
    FB_DO(c.end());
    FB_DO(c.download());
    std::memcpy(post, c.host.data() + o_out, 8 * (size_t)n);
    fb->post_ms[0] = c.ms(0);
    return PAGAN_OK;
}

// The two marginal passes over n handles of one device: one launch per pass, grid = (blocks of the longest pair, pairs that want
// the pass).  o[0..3] rows (pX, pM, best_j, best_p), o[4..7] columns (pY, pM', best_i, best_p'): arrays of n pointers or null,
// any entry null.  A pass none of whose outputs is wanted anywhere is not launched.  A pass's time goes to the first handle that
// wanted it.
static int fb_marginals(int32_t n, pagan_fb *const *fbs, void *const *const o[8]) {
    if (n < 0 || (n > 0 && !fbs)) return PAGAN_E_ARG;
    if (n == 0) return PAGAN_OK;
    FbCall c;
    FB_DO(c.open(n, fbs));
    auto wanted = [&](int k, int side) { for (int q = 4 * side; q < 4 * side + 4; ++q) if (o[q] && o[q][k]) return true; return false; };
    struct Side { std::vector<int> ks; std::vector<size_t> at; int blocks = 0; size_t o_jobs = 0, o_recs = 0; };
    Side sd[2];
    for (int side = 0; side < 2; ++side) {
        for (int k = 0; k < n; ++k) if (wanted(k, side)) sd[side].ks.push_back(k);
        sd[side].o_jobs = c.take(FbCall::UP, sd[side].ks.size() * sizeof(PgFbJob));
        sd[side].o_recs = c.take(FbCall::UP, sd[side].ks.size() * sizeof(PgFbMarg));
    }
    for (int side = 0; side < 2; ++side)
        for (int k : sd[side].ks) {
            const int len = side ? fbs[k]->Ly : fbs[k]->Lx;
            sd[side].at.push_back(c.take(FbCall::DOWN, 28 * (size_t)len));          // three doubles and an int a site
            sd[side].blocks = std::max(sd[side].blocks, (len + FB_PM_ROWS - 1) / FB_PM_ROWS);
        }
    if (sd[0].ks.empty() && sd[1].ks.empty()) return PAGAN_OK;
    FB_DO(c.alloc());
    for (int side = 0; side < 2; ++side)
        for (size_t q = 0; q < sd[side].ks.size(); ++q) {
            const pagan_fb *fb = fbs[sd[side].ks[q]];
            const size_t len = side ? fb->Ly : fb->Lx;
            char *base = c.dev<char>(sd[side].at[q]);
            PgFbMarg M;
            M.gap = (double *)base; M.match = (double *)(base + 8 * len); M.best_p = (double *)(base + 16 * len); M.best = (int *)(base + 24 * len);
            c.put(sd[side].o_jobs + q * sizeof(PgFbJob), fb->job);
            c.put(sd[side].o_recs + q * sizeof(PgFbMarg), M);
        }
    FB_DO(c.upload());
    for (int side = 0; side < 2; ++side) {
        if (sd[side].ks.empty()) continue;
        FB_DO(c.begin());
        const dim3 grid((unsigned)sd[side].blocks, (unsigned)sd[side].ks.size());
        const PgFbJob *jobs = c.dev<const PgFbJob>(sd[side].o_jobs);
        const PgFbMarg *recs = c.dev<const PgFbMarg>(sd[side].o_recs);
        if (side) hipLaunchKernelGGL((pg_fb_marginals<true>), grid, dim3(FB_PM_ROWS), 0, nullptr, jobs, recs);
        else hipLaunchKernelGGL((pg_fb_marginals<false>), grid, dim3(FB_PM_ROWS), 0, nullptr, jobs, recs);
        FB_DO(c.end());
    }
    FB_DO(c.download());
    for (int k = 0; k < n; ++k) fbs[k]->post_ms[1] = fbs[k]->post_ms[2] = 0.0f;
    for (int side = 0; side < 2; ++side) {
        if (sd[side].ks.empty()) continue;
        fbs[sd[side].ks[0]]->post_ms[1 + side] = c.ms(side && !sd[0].ks.empty() ? 1 : 0);   // (spans in the order of the passes launched)
        for (size_t q = 0; q < sd[side].ks.size(); ++q) {
            const int k = sd[side].ks[q];
            const size_t len = side ? fbs[k]->Ly : fbs[k]->Lx;
            const char *base = c.host.data() + sd[side].at[q];
            void *const *const *oo = o + 4 * side;
            if (oo[0] && oo[0][k]) std::memcpy(oo[0][k], base, 8 * len);
            if (oo[1] && oo[1][k]) std::memcpy(oo[1][k], base + 8 * len, 8 * len);
            if (oo[2] && oo[2][k]) std::memcpy(oo[2][k], base + 24 * len, 4 * len);
            if (oo[3] && oo[3][k]) std::memcpy(oo[3][k], base + 16 * len, 8 * len);
        }
    }
    return PAGAN_OK;
}

// The expected counts of n handles of one device: pg_fb_counts over (work items of the longest pair, pairs), then pg_fb_counts_fold,
// one workgroup a pair.  One buffer: the job records, the count records, the pairs' work items, then per pair the result and the
// work items' partial sums.  The time goes to fbs[0].
static size_t fb_counts_stride(const pagan_fb *fb, bool emit) { return 9 + (emit ? (size_t)fb->S * fb->S : 0); }
// A pair's work items (first row of a row block, first diagonal, last diagonal + 1): per block of FB_CN_ROWS rows the diagonals that
// hold a cell of the block -- for a monotone band imin and imax never fall (dp_band.h) --, in segments of FB_CN_SEG
static void fb_counts_items(const pagan_fb *fb, std::vector<int> *items) {
    const DiagIndex &dx = fb->dx;
    const int nd = fb->Lx + fb->Ly - 1;
    int d0 = 0, d1 = 0;
    for (int r0 = 0; r0 < fb->Lx; r0 += FB_CN_ROWS) {
        const int r1 = std::min(fb->Lx, r0 + FB_CN_ROWS) - 1;
        while (d0 < nd && dx.imax[d0] < r0) ++d0;                  // the first diagonal whose last row is >= r0
        d1 = std::max(d1, d0);
        while (d1 < nd && dx.imin[d1] <= r1) ++d1;                 // the first diagonal whose first row is > r1
        for (int d = d0; d < d1; d += FB_CN_SEG) { items->push_back(r0); items->push_back(d); items->push_back(std::min(d + FB_CN_SEG, d1)); }
    }
}
static int fb_counts(int32_t n, pagan_fb *const *fbs, double *const *trans, double *const *emit) {
    if (n < 0 || (n > 0 && (!fbs || !trans))) return PAGAN_E_ARG;
    for (int k = 0; k < n; ++k)
        if (!fbs[k] || !trans[k] || (emit && emit[k] && fbs[k]->S > FB_CN_MAXS)) return PAGAN_E_ARG;
    if (n == 0) return PAGAN_OK;
    FbCall c;
    FB_DO(c.open(n, fbs));
    const size_t o_jobs = c.take(FbCall::UP, (size_t)n * sizeof(PgFbJob)), o_recs = c.take(FbCall::UP, (size_t)n * sizeof(PgFbCounts));
    std::vector<std::vector<int>> items(n);
    std::vector<size_t> o_items(n), o_out(n), o_part(n);
    int widest = 0;
    size_t lds = 0;
    for (int k = 0; k < n; ++k) {
        fb_counts_items(fbs[k], &items[k]);
        o_items[k] = c.take(FbCall::UP, 4 * items[k].size());
        widest = std::max(widest, (int)(items[k].size() / 3));
        if (emit && emit[k]) lds = std::max(lds, 8 * (size_t)FB_CN_ROWS * fbs[k]->S);
    }
    for (int k = 0; k < n; ++k) o_out[k] = c.take(FbCall::DOWN, 8 * (fb_counts_stride(fbs[k], emit && emit[k]) + 3));
    for (int k = 0; k < n; ++k) o_part[k] = c.take(FbCall::DEVICE, 8 * fb_counts_stride(fbs[k], emit && emit[k]) * (items[k].size() / 3));
    FB_DO(c.alloc());
    for (int k = 0; k < n; ++k) {
        PgFbCounts R;
        R.part = c.dev<double>(o_part[k]); R.out = c.dev<double>(o_out[k]);
        R.items = c.dev<const int>(o_items[k]); R.n_items = (int)(items[k].size() / 3); R.emit = emit && emit[k] ? 1 : 0;
        c.put(o_jobs + k * sizeof(PgFbJob), fbs[k]->job);
        c.put(o_recs + k * sizeof(PgFbCounts), R);
        if (!items[k].empty()) std::memcpy(c.host.data() + o_items[k], items[k].data(), 4 * items[k].size());
    }
    FB_DO(c.upload());
    const PgFbJob *jobs = c.dev<const PgFbJob>(o_jobs);
    const PgFbCounts *recs = c.dev<const PgFbCounts>(o_recs);
    FB_DO(c.begin());
    if (widest > 0) hipLaunchKernelGGL(pg_fb_counts, dim3((unsigned)widest, (unsigned)n), dim3(FB_CN_ROWS), lds, nullptr, jobs, recs);
    hipLaunchKernelGGL(pg_fb_counts_fold, dim3((unsigned)n), dim3(256), 0, nullptr, jobs, recs);
    FB_DO(c.end());
    FB_DO(c.download());
    for (int k = 0; k < n; ++k) fbs[k]->counts_ms = 0.0f;
    fbs[0]->counts_ms = c.ms(0);
    for (int k = 0; k < n; ++k) {
        std::memcpy(trans[k], c.host.data() + o_out[k], 8 * 12);
        if (emit && emit[k]) std::memcpy(emit[k], c.host.data() + o_out[k] + 8 * 12, 8 * (size_t)fbs[k]->S * fbs[k]->S);
    }
    return PAGAN_OK;
}

static uint64_t fb_splitmix64(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

// The result of a pair whose full probability is 0: nothing to sample, nothing to decode
static int fb_unreachable_result(const pagan_graph *L, const pagan_graph *R, long long cells, double log_fwd, pagan_result *out) {
    int endcell[8] = {1, 0, 0, 0, -1, -1, 0, 0};
    return pagan_internal_replay(L, R, cells, endcell, log_fwd, nullptr, out);
}
// A trace's first n records as `visited` has them: (i, j, state)
static void fb_visited_of(const int *trace, int n, int32_t *visited) {
    for (int t = 0; t < n; ++t) { visited[3 * t] = trace[3 * t]; visited[3 * t + 1] = trace[3 * t + 1]; visited[3 * t + 2] = trace[3 * t + 2] & 3; }
}
} // namespace

extern "C" {

// Posterior of n cells given as (state, i, j) triples: one upload, pg_fb_gather, one download.
int pagan_fb_posterior_cells(pagan_fb *fb, int32_t n, const int32_t *cells, double *post) {
    if (!fb || n < 0 || (n > 0 && (!cells || !post))) return PAGAN_E_ARG;
    for (int k = 0; k < n; ++k) if (cells[3 * k] < 0 || cells[3 * k] > 2) return PAGAN_E_ARG;
    return fb_gather(fb, n, cells, post);
}

// Host only: the DP cell every column of a path sits on (include/pagan_dp.h).
int pagan_path_cells(const pagan_col *cols, int32_t n_cols, int32_t *cells) {
    if (n_cols < 0 || (n_cols > 0 && (!cols || !cells))) return PAGAN_E_ARG;
    int ci = 0, cj = 0;
    for (int k = 0; k < n_cols; ++k) {
        int s = -1, i = -1, j = -1;
        switch (cols[k].path_state) {
        case PAGAN_MATCHED: ci = cols[k].left; cj = cols[k].right; s = PAGAN_M_MAT; i = ci; j = cj; break;
        case PAGAN_XGAPPED: ci = cols[k].left; s = PAGAN_X_MAT; i = ci; j = cj; break;
        case PAGAN_YGAPPED: cj = cols[k].right; s = PAGAN_Y_MAT; i = ci; j = cj; break;
        case PAGAN_XSKIPPED: case PAGAN_YSKIPPED: break;
        default: return PAGAN_E_ARG;
        }
        cells[3 * k] = s; cells[3 * k + 1] = i; cells[3 * k + 2] = j;
    }
    return PAGAN_OK;
}

int pagan_fb_path_support(pagan_fb *fb, const pagan_col *cols, int32_t n_cols, double *support) {
    if (!fb || n_cols < 0 || (n_cols > 0 && (!cols || !support))) return PAGAN_E_ARG;
    std::vector<int32_t> cells(3 * (size_t)n_cols);
    const int rc = pagan_path_cells(cols, n_cols, cells.data());
    if (rc != PAGAN_OK) return rc;
    for (int k = 0; k < n_cols; ++k)
        if (cells[3 * k] >= 0 && (cells[3 * k + 1] < 0 || cells[3 * k + 1] >= fb->Lx || cells[3 * k + 2] < 0 || cells[3 * k + 2] >= fb->Ly)) return PAGAN_E_ARG;
    return fb_gather(fb, n_cols, cells.data(), support);
}

int pagan_fb_site_marginals_batch(int32_t n, pagan_fb *const *fbs, double *const *pX, double *const *pM_left, int32_t *const *best_j,
                                  double *const *best_p_left, double *const *pY, double *const *pM_right, int32_t *const *best_i,
                                  double *const *best_p_right) {
    void *const *const o[8] = {(void *const *)pX, (void *const *)pM_left, (void *const *)best_j, (void *const *)best_p_left,
                               (void *const *)pY, (void *const *)pM_right, (void *const *)best_i, (void *const *)best_p_right};
    return fb_marginals(n, fbs, o);
}

int pagan_fb_site_marginals(pagan_fb *fb, double *pX, double *pM_left, int32_t *best_j, double *best_p_left, double *pY,
                            double *pM_right, int32_t *best_i, double *best_p_right) {
    if (!fb) return PAGAN_E_ARG;
    return pagan_fb_site_marginals_batch(1, &fb, &pX, &pM_left, &best_j, &best_p_left, &pY, &pM_right, &best_i, &best_p_right);
}

int pagan_fb_post_ms(const pagan_fb *fb, double ms[3]) {
    if (!fb || !ms) return PAGAN_E_ARG;
    for (int k = 0; k < 3; ++k) ms[k] = fb->post_ms[k];
    return PAGAN_OK;
}

// Expected transition and emission counts (dp_fb_counts.inc; include/pagan_dp.h has the definitions).
int pagan_fb_expected_counts_batch(int32_t n, pagan_fb *const *fbs, double *const *trans, double *const *emit) {
    return fb_counts(n, fbs, trans, emit);
}

int pagan_fb_expected_counts(pagan_fb *fb, double trans[12], double *emit) {
    if (!fb || !trans) return PAGAN_E_ARG;
    return fb_counts(1, &fb, &trans, &emit);
}

int pagan_fb_counts_ms(const pagan_fb *fb, double *ms) {
    if (!fb || !ms) return PAGAN_E_ARG;
    *ms = fb->counts_ms;
    return PAGAN_OK;
}

// What fb_counts allocates for a pair, from above: a row block of 64 rows crosses at most right_sites + 62 diagonals, in segments
// of FB_CN_SEG (a tunnel's row block crosses far fewer); per work item the partial sums (8 B an entry) and 12 B of the item
// itself, then the result and the two records.
int64_t pagan_fb_counts_predict_bytes(int32_t left_sites, int32_t right_sites, int32_t n_states) {
    if (left_sites < 2 || right_sites < 2 || n_states < 1) return PAGAN_E_ARG;
    const int64_t stride = 9 + (n_states <= FB_CN_MAXS ? (int64_t)n_states * n_states : 0);
    const int64_t nb = ((int64_t)left_sites - 1 + FB_CN_ROWS - 1) / FB_CN_ROWS;
    const int64_t segs = ((int64_t)right_sites - 1 + FB_CN_ROWS - 1 + FB_CN_SEG - 1) / FB_CN_SEG;
    return (8 * stride + 12) * nb * segs + 8 * (stride + 3) + (int64_t)sizeof(PgFbJob) + (int64_t)sizeof(PgFbCounts) + 5 * 256;
}

// u[s] = (mix(mix(mix(seed) ^ node) ^ s) >> 11) * 2^-53, mix = splitmix64's output function of x + 0x9E3779B97F4A7C15
int pagan_sample_uniforms(uint64_t seed, int32_t node, int32_t n, double *u) {
    if (n < 0 || (n > 0 && !u)) return PAGAN_E_ARG;
    const uint64_t key = fb_splitmix64(fb_splitmix64(seed) ^ (uint64_t)(int64_t)node);
    for (int s = 0; s < n; ++s) u[s] = (double)(fb_splitmix64(key ^ (uint64_t)s) >> 11) * (1.0 / 9007199254740992.0);
    return PAGAN_OK;
}

// The stream of path `path` of a node: the counter of pagan_sample_uniforms with the path in its upper half,
// u[s] = (mix(key ^ (s + (path << 32))) >> 11) * 2^-53 -- path 0 is pagan_sample_uniforms bit for bit.  pg_fb_sample computes the
// same numbers from (key, path, s) where it uses them (dp_fb_sample.inc, fs_uniform).
int pagan_sample_uniforms_path(uint64_t seed, int32_t node, int32_t path, int32_t n, double *u) {
    if (path < 0 || n < 0 || (n > 0 && !u)) return PAGAN_E_ARG;
    const uint64_t key = fb_splitmix64(fb_splitmix64(seed) ^ (uint64_t)(int64_t)node);
    for (int s = 0; s < n; ++s) u[s] = (double)(fb_splitmix64(key ^ ((uint64_t)s + ((uint64_t)path << 32))) >> 11) * (1.0 / 9007199254740992.0);
    return PAGAN_OK;
}

// sample_new_path (VA:1193-1322): a path drawn from the posterior by walking back from the end corner; at every step
// the predecessors are listed in the forward pass's candidate order with weight fwd(pred) * transition (add_sample_*,
// VA:2309-2446) and the first one whose running sum reaches u * total is taken (VA:1757-1769).  u[k] in [0, 1) stands
// for rand()/(RAND_MAX+1): one number per step, the end corner first (at most Lx + Ly + 1 are used).  The result has
// the shape of a Viterbi result (columns, used edges; score = log of the full probability).  visited (optional,
// 3 * (Lx + Ly) ints): the cells of the path end -> start as (i, j, state).
int pagan_fb_sample_path(pagan_fb *fb, const double *u, int32_t n_u, pagan_result *out, int32_t *visited, int32_t *n_visited) {
    if (!fb || !u || !out) return PAGAN_E_ARG;
    DeviceScope on_device(fb->device);
    if (!on_device.ok) return PAGAN_E_NODEVICE;
    if (fb->hF.empty()) {
        fb->hF.resize(3 * (size_t)fb->dx.cells);
        FB_TRY(hipMemcpy(fb->hF.data(), fb->dF, 8 * fb->hF.size(), hipMemcpyDeviceToHost));
    }
    const pagan_graph *L = fb->L, *R = fb->R;
    const int Lx = fb->Lx, Ly = fb->Ly, S = fb->S;
    auto F = [&](int s, int i, int j) { const long long a = fb->at(i, j); return a < 0 ? -HUGE_VAL : fb->hF[3 * a + s]; };
    const double ext = std::log((double)fb->gap_ext), open = std::log((double)fb->gap_open), ng = std::log((double)fb->non_gap);
    struct Cand { double lw; int state, i, j, k1, k2; };
    std::vector<Cand> c;
    auto pick = [&](double uu) -> int {
        double hi = -HUGE_VAL;
        for (const Cand &x : c) hi = std::max(hi, x.lw);
        if (c.empty() || hi == -HUGE_VAL) return -1;
        double tot = 0;
        for (const Cand &x : c) tot += std::exp(x.lw - hi);
        const double rv = tot * uu;
        size_t k = 0;
        double sum = std::exp(c[0].lw - hi);
        while (sum < rv && k + 1 < c.size()) { ++k; sum += std::exp(c[k].lw - hi); }
        return (int)k;
    };
    int used = 0;
    {   // iterate_bwd_edges_for_sampled_end_corner, VA:1904-2025
        const int l0 = L->bwd_off[Lx], l1 = L->bwd_off[Lx + 1], r0 = R->bwd_off[Ly], r1 = R->bwd_off[Ly + 1];
        auto mt = [&](int k1, int k2) { c.push_back({F(2, L->bwd_src[k1], R->bwd_src[k2]) + ng + (double)L->bwd_logw[k1] + (double)R->bwd_logw[k2], 2, L->bwd_src[k1], R->bwd_src[k2], k1 - l0, k2 - r0}); };
        auto xc = [&](int k1) { c.push_back({F(0, L->bwd_src[k1], Ly - 1), 0, L->bwd_src[k1], Ly - 1, k1 - l0, -1}); };
        auto yc = [&](int k2) { c.push_back({F(1, Lx - 1, R->bwd_src[k2]), 1, Lx - 1, R->bwd_src[k2], -1, k2 - r0}); };
        if (l1 > l0 && r1 > r0) {
            mt(l0, r0); xc(l0); yc(r0);
            for (int k2 = r0 + 1; k2 < r1; ++k2) { mt(l0, k2); yc(k2); }
            for (int k1 = l0 + 1; k1 < l1; ++k1) { mt(k1, r0); xc(k1); for (int k2 = r0 + 1; k2 < r1; ++k2) { mt(k1, k2); yc(k2); } }
        }
    }
    if (used >= n_u) return PAGAN_E_ARG;
    int k = pick(u[used++]);
    if (k < 0) return fb_unreachable_result(L, R, fb->dx.cells, fb->totals[0], out);
    int endcell[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    int state = c[k].state, i = c[k].i, j = c[k].j;
    endcell[1] = state; endcell[2] = i; endcell[3] = j; endcell[4] = c[k].k1; endcell[5] = c[k].k2;
    std::vector<int> trace;
    trace.reserve(3 * ((size_t)Lx + Ly));
    while (!(i < 1 && j < 1)) {
        c.clear();
        if (state == 2) {
            const double sc = std::log((double)fb->score[L->state[i] + (size_t)R->state[j] * S]);
            for (int k1 = L->bwd_off[i]; k1 < L->bwd_off[i + 1]; ++k1)
                for (int k2 = R->bwd_off[j]; k2 < R->bwd_off[j + 1]; ++k2) {
                    const int p = L->bwd_src[k1], q = R->bwd_src[k2];
                    const double w = (double)L->bwd_logw[k1] + (double)R->bwd_logw[k2];
                    const int a = k1 - L->bwd_off[i], b = k2 - R->bwd_off[j];
                    c.push_back({F(2, p, q) + ng + ng + sc + w, 2, p, q, a, b});
                    c.push_back({F(0, p, q) + ng + sc + w, 0, p, q, a, b});
                    c.push_back({F(1, p, q) + ng + sc + w, 1, p, q, a, b});
                }
        } else if (state == 0) {
            for (int k1 = L->bwd_off[i]; k1 < L->bwd_off[i + 1]; ++k1) {
                const int p = L->bwd_src[k1], a = k1 - L->bwd_off[i];
                c.push_back({F(0, p, j) + ext, 0, p, j, a, 0}); c.push_back({F(1, p, j) + open, 1, p, j, a, 0});
                c.push_back({F(2, p, j) + ng + open, 2, p, j, a, 0});
            }
        } else {
            for (int k2 = R->bwd_off[j]; k2 < R->bwd_off[j + 1]; ++k2) {
                const int q = R->bwd_src[k2], b = k2 - R->bwd_off[j];
                c.push_back({F(1, i, q) + ext, 1, i, q, 0, b}); c.push_back({F(0, i, q) + open, 0, i, q, 0, b});
                c.push_back({F(2, i, q) + ng + open, 2, i, q, 0, b});
            }
        }
        if (used >= n_u) return PAGAN_E_ARG;
        k = pick(u[used++]);
        if (k < 0 || (size_t)trace.size() >= 3 * ((size_t)Lx + Ly)) return PAGAN_E_INTERNAL;
        trace.push_back(i); trace.push_back(j);
        trace.push_back((int)((unsigned)state | ((unsigned)c[k].k1 << 4) | ((unsigned)c[k].k2 << 18)));
        state = c[k].state; i = c[k].i; j = c[k].j;
    }
    endcell[6] = (int)(trace.size() / 3);
    if (visited) fb_visited_of(trace.data(), endcell[6], visited);
    if (n_visited) *n_visited = endcell[6];
    trace.resize(trace.size() + 3, 0);
    return pagan_internal_replay(L, R, fb->dx.cells, endcell, fb->totals[0], trace.data(), out);
}

} // extern "C"

// ---- paths on the device: K sampled per pair (pg_fb_sample, dp_fb_sample.inc), or the decoded one (dp_fb_decode.inc) ----
// One allocation serves a whole batch call -- the job records, the launch records, every pair's summaries, traces and pack
// buffer -- and lives as long as any of the batch's handles does.  What the two handles share: the pair they are paths of, the
// traces on the device, a summary per path, and the three ways of reading a path.

struct FbPaths {
    int device = 0;
    int Lx = 0, Ly = 0, n_paths = 1, max_steps = 0;
    uint32_t flags = 0;
    const pagan_graph *L = nullptr, *R = nullptr;       // borrowed from the pagan_fb: must outlive the handle for result()
    long long cells = 0;
    double log_fwd = 0;
    std::shared_ptr<DevBuf> buf;
    const int *d_trace = nullptr;                       // [group][step][lane of the group][3]; null: PAGAN_SAMPLE_NO_TRACES
    int *d_pack = nullptr;                              // [max_steps][3]: one path out of a group of several (n_paths > 1)
    std::mutex pack_mu;
    std::vector<int32_t> summary;                       // [n_paths][FB_SUMMARY_INTS], downloaded by the batch call

    void bind(const pagan_fb *fb, int paths, uint32_t flags_, const FbCall &c) {
        device = fb->device; Lx = fb->Lx; Ly = fb->Ly; n_paths = paths; max_steps = Lx + Ly; flags = flags_;
        L = fb->L; R = fb->R; cells = fb->dx.cells; log_fwd = fb->totals[0];
        buf = c.buf;
    }
    void keep_summary(const FbCall &c, size_t off) {
        const int32_t *sm = (const int32_t *)(c.host.data() + off);
        summary.assign(sm, sm + (size_t)FB_SUMMARY_INTS * n_paths);
    }
    const int32_t *sum(int path) const { return summary.data() + (size_t)FB_SUMMARY_INTS * path; }
    // the steps of a path; of one that is none (status 1 or 2): 0
    int steps(int path) const { return sum(path)[FB_SUM_STATUS] == 0 ? sum(path)[FB_SUM_STEPS] : 0; }
    double value(int path) const { double v; std::memcpy(&v, sum(path) + FB_SUM_VALUE, 8); return v; }

    // path `path`'s records, contiguous, three zero ints behind them (pagan_internal_replay's format)
    int fetch(int path, std::vector<int> *trace, int *n_steps) {
        const int n = steps(path);
        if (n < 0 || n > max_steps) return PAGAN_E_INTERNAL;
        trace->assign(3 * ((size_t)n + 1), 0);
        *n_steps = n;
        if (n == 0) return PAGAN_OK;
        DeviceScope on_device(device);
        if (!on_device.ok) return PAGAN_E_NODEVICE;
        const int g = path / 64, lane = path % 64, width = std::min(64, n_paths - 64 * g);
        const int *group = d_trace + 3 * (64ll * g * max_steps);
        if (width == 1) {                                   // (one path a group: its records are one run already)
            FB_TRY(hipMemcpy(trace->data(), group, 12 * (size_t)n, hipMemcpyDeviceToHost));
            return PAGAN_OK;
        }
        std::lock_guard<std::mutex> lock(pack_mu);
        hipLaunchKernelGGL(pg_fb_trace_pack, dim3((unsigned)std::min((n + 255) / 256, 1024)), dim3(256), 0, nullptr, group, width, lane, n, d_pack);
        FB_TRY(hipGetLastError());
        FB_TRY(hipMemcpy(trace->data(), d_pack, 12 * (size_t)n, hipMemcpyDeviceToHost));
        return PAGAN_OK;
    }
    // the path's cells end -> start as (i, j, state), 3 * (Lx + Ly) ints at most: pagan_fb_sample_path's `visited`
    int visited(int path, int32_t *visited, int32_t *n_visited) {
        std::vector<int> trace;
        int n = 0;
        FB_DO(fetch(path, &trace, &n));
        fb_visited_of(trace.data(), n, visited);
        if (n_visited) *n_visited = n;
        return PAGAN_OK;
    }
    // the replay of one trace: pagan_fb_sample_path's result (score = log full probability; status 1: the unreachable result)
    int result(int path, pagan_result *out) {
        const int32_t *sm = sum(path);
        if (sm[FB_SUM_STATUS] == 1) return fb_unreachable_result(L, R, cells, log_fwd, out);
        if (sm[FB_SUM_STATUS] != 0) return PAGAN_E_INTERNAL;
        std::vector<int> trace;
        int endcell[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        FB_DO(fetch(path, &trace, &endcell[6]));
        for (int k = 0; k < 5; ++k) endcell[1 + k] = sm[FB_SUM_END + k];
        return pagan_internal_replay(L, R, cells, endcell, log_fwd, trace.data(), out);
    }
};

struct pagan_fb_samples : FbPaths {
    float ms = 0;                                       // pg_fb_sample (HIP events), at the batch's first pair
};

namespace {
// bytes of one pair's part of the allocation: summaries, traces, pack buffer (each rounded up to 256)
struct FsSizes { size_t summary, trace, pack; };
static FsSizes fs_sizes(int Lx, int Ly, int n_paths, uint32_t flags) {
    const size_t steps = (size_t)Lx + Ly;
    const bool traces = !(flags & PAGAN_SAMPLE_NO_TRACES);
    return {up256(4 * (size_t)FB_SUMMARY_INTS * n_paths), traces ? up256(12 * (size_t)n_paths * steps) : 0,
            traces && n_paths > 1 ? up256(12 * steps) : 0};
}
} // namespace

extern "C" {

// n_paths paths for each of n pairs of one device in one launch: grid = (groups of 64 paths, pairs).  The summaries come back
// with the call; the traces stay on the device until somebody asks for a path (pagan_fb_samples_visited / _result).
int pagan_fb_sample_paths_batch(int32_t n, pagan_fb *const *fbs, uint64_t seed, const int32_t *nodes, int32_t n_paths, uint32_t flags,
                                pagan_fb_samples **out) {
    if (n < 0 || n_paths < 1 || (flags & ~PAGAN_SAMPLE_NO_TRACES) || (n > 0 && (!fbs || !nodes || !out))) return PAGAN_E_ARG;
    for (int k = 0; k < n; ++k) out[k] = nullptr;
    if (n == 0) return PAGAN_OK;
    FbCall c;
    FB_DO(c.open(n, fbs));
    const size_t o_jobs = c.take(FbCall::UP, (size_t)n * sizeof(PgFbJob)), o_recs = c.take(FbCall::UP, (size_t)n * sizeof(PgFbSample));
    std::vector<size_t> o_sum(n), o_trace(n), o_pack(n);
    for (int k = 0; k < n; ++k) o_sum[k] = c.take(FbCall::DOWN, fs_sizes(fbs[k]->Lx, fbs[k]->Ly, n_paths, flags).summary);
    for (int k = 0; k < n; ++k) {
        const FsSizes z = fs_sizes(fbs[k]->Lx, fbs[k]->Ly, n_paths, flags);
        o_trace[k] = c.take(FbCall::DEVICE, z.trace); o_pack[k] = c.take(FbCall::DEVICE, z.pack);
    }
    FB_DO(c.alloc());
    const bool traces = !(flags & PAGAN_SAMPLE_NO_TRACES);
    const int groups = (n_paths + 63) / 64;
    for (int k = 0; k < n; ++k) {
        PgFbSample R;
        R.key = fb_splitmix64(fb_splitmix64(seed) ^ (uint64_t)(int64_t)nodes[k]);
        R.n_paths = n_paths; R.groups = groups; R.max_steps = fbs[k]->Lx + fbs[k]->Ly; R.pad = 0;
        R.trace = traces ? c.dev<int>(o_trace[k]) : nullptr;
        R.summary = c.dev<int>(o_sum[k]);
        c.put(o_jobs + (size_t)k * sizeof(PgFbJob), fbs[k]->job);
        c.put(o_recs + (size_t)k * sizeof(PgFbSample), R);
    }
    FB_DO(c.upload());
    FB_DO(c.begin());
    for (int at = 0; at < n; at += 65535) {                    // (a grid's y extent)
        const dim3 grid((unsigned)groups, (unsigned)std::min(65535, n - at));
        hipLaunchKernelGGL(pg_fb_sample, grid, dim3(64), 0, nullptr, c.dev<const PgFbJob>(o_jobs) + at, c.dev<const PgFbSample>(o_recs) + at);
    }
    FB_DO(c.end());
    FB_DO(c.download());
    for (int k = 0; k < n; ++k) {
        pagan_fb_samples *s = new pagan_fb_samples();
        s->bind(fbs[k], n_paths, flags, c);
        s->d_trace = traces ? c.dev<const int>(o_trace[k]) : nullptr;
        s->d_pack = traces && n_paths > 1 ? c.dev<int>(o_pack[k]) : nullptr;
        s->keep_summary(c, o_sum[k]);
        s->ms = k == 0 ? c.ms(0) : 0.0f;
        out[k] = s;
    }
    return PAGAN_OK;
}

int pagan_fb_sample_paths(pagan_fb *fb, uint64_t seed, int32_t node, int32_t n_paths, uint32_t flags, pagan_fb_samples **out) {
    if (!fb || !out) return PAGAN_E_ARG;
    return pagan_fb_sample_paths_batch(1, &fb, seed, &node, n_paths, flags, out);
}

int pagan_fb_samples_summary(const pagan_fb_samples *s, int32_t *status, int32_t *n_steps, int32_t *n_m, int32_t *n_x, int32_t *n_y,
                             double *log_q) {
    if (!s) return PAGAN_E_ARG;
    for (int p = 0; p < s->n_paths; ++p) {
        const int32_t *sm = s->sum(p);
        if (status) status[p] = sm[FB_SUM_STATUS];
        if (n_steps) n_steps[p] = sm[FB_SUM_STEPS];
        if (n_m) n_m[p] = sm[FB_SUM_M];
        if (n_x) n_x[p] = sm[FB_SUM_X];
        if (n_y) n_y[p] = sm[FB_SUM_Y];
        if (log_q) log_q[p] = s->value(p);
    }
    return PAGAN_OK;
}

int pagan_fb_samples_visited(pagan_fb_samples *s, int32_t path, int32_t *visited, int32_t *n_visited) {
    if (!s || !s->d_trace || path < 0 || path >= s->n_paths || !visited) return PAGAN_E_ARG;
    return s->visited(path, visited, n_visited);
}

// every path's cells in ONE copy of the trace buffer: visited [n_paths][Lx + Ly][3] (rows behind a path's last step: 0),
// n_visited [n_paths]
int pagan_fb_samples_visited_all(pagan_fb_samples *s, int32_t *visited, int32_t *n_visited) {
    if (!s || !s->d_trace || !visited) return PAGAN_E_ARG;
    DeviceScope on_device(s->device);
    if (!on_device.ok) return PAGAN_E_NODEVICE;
    const size_t ms = (size_t)s->max_steps;
    std::vector<int32_t> raw(3 * (size_t)s->n_paths * ms);
    if (!raw.empty()) FB_TRY(hipMemcpy(raw.data(), s->d_trace, 4 * raw.size(), hipMemcpyDeviceToHost));
    for (int p = 0; p < s->n_paths; ++p) {
        const int n = s->steps(p);
        if (n < 0 || n > s->max_steps) return PAGAN_E_INTERNAL;
        const int g = p / 64, lane = p % 64, width = std::min(64, s->n_paths - 64 * g);
        const int32_t *group = raw.data() + 3 * (64 * (size_t)g * ms);
        int32_t *o = visited + 3 * (size_t)p * ms;
        for (int t = 0; t < n; ++t) {
            const int32_t *r = group + 3 * ((size_t)t * width + lane);
            o[3 * t] = r[0]; o[3 * t + 1] = r[1]; o[3 * t + 2] = r[2] & 3;
        }
        std::memset(o + 3 * (size_t)n, 0, 12 * (ms - (size_t)n));
        if (n_visited) n_visited[p] = n;
    }
    return PAGAN_OK;
}

int pagan_fb_samples_result(pagan_fb_samples *s, int32_t path, pagan_result *out) {
    if (!s || !s->d_trace || path < 0 || path >= s->n_paths || !out) return PAGAN_E_ARG;
    return s->result(path, out);
}

int pagan_fb_samples_ms(const pagan_fb_samples *s, double *ms) {
    if (!s || !ms) return PAGAN_E_ARG;
    *ms = s->ms;
    return PAGAN_OK;
}

// What pagan_fb_sample_paths_batch allocates for one pair: 12 B a path step (and one path's pack buffer when a group holds
// several), 64 B a path of summary, the records.  The matrix is the pagan_fb's: nothing here grows with Lx * Ly.
int64_t pagan_fb_sample_predict_bytes(int32_t left_sites, int32_t right_sites, int32_t n_paths, uint32_t flags) {
    if (left_sites < 2 || right_sites < 2 || n_paths < 1 || (flags & ~PAGAN_SAMPLE_NO_TRACES)) return PAGAN_E_ARG;
    const FsSizes z = fs_sizes(left_sites - 1, right_sites - 1, n_paths, flags);
    return (int64_t)(z.summary + z.trace + z.pack + sizeof(PgFbJob) + sizeof(PgFbSample) + 1024);
}

void pagan_fb_samples_destroy(pagan_fb_samples *s) { delete s; }

void pagan_fb_destroy(pagan_fb *fb) {
    if (!fb) return;
    give_slab(fb_arena_pool, fb->device, fb->arena, fb->arena_cap);
    delete fb;
}

} // extern "C"

// ---- posterior decoding: the maximum expected accuracy path of a finished pass (dp_fb_decode.inc) ----
// A pair's score matrix A (24 B a cell) is an arena of its own from fb_arena_pool: it goes back to the pool behind the trace
// unless the caller keeps it (PAGAN_DECODE_KEEP_MATRIX).  The handle is a path handle of one path, [max_steps][3].

struct pagan_fb_decoded : FbPaths {
    DiagIndex dx;                                       // kept matrix only: where a cell sits (pagan_fb_decoded_dump)
    char *arena = nullptr;                              // A; null once it went back to the pool
    size_t arena_cap = 0;
    float ms[2] = {0, 0};                               // fill, trace (HIP events), at the batch's first pair
    int schedule = 0;                                   // 0 pg_fb_decode_fill, 1 pg_fb_ring_decode
    int threads = 0, tab = 0;                           // the fill launch's workgroup size; the ring instance looked the table up
    ~pagan_fb_decoded() { give_slab(fb_arena_pool, device, arena, arena_cap); }
};

namespace {
// bytes a pair's decode takes: the matrix A (an arena of the pool's), and of the call's allocation the summary and the trace
struct FdSizes { size_t matrix, summary, trace; };
static FdSizes fd_sizes(long long cells, int Lx, int Ly) {
    return {24 * (size_t)cells, up256(4 * FB_SUMMARY_INTS), up256(12 * ((size_t)Lx + Ly))};
}
// waits for the default stream when a call leaves, by whichever return: a handle's matrix must not reach fb_arena_pool (whose next
// take would hand it out) while a kernel may still be writing it
struct FdStreamWait { ~FdStreamWait() { (void)hipStreamSynchronize(nullptr); } };
} // namespace

extern "C" {

// The decode of n finished pairs of one device: the fills (one launch of pg_fb_decode_fill over the fill pairs, one of
// pg_fb_ring_decode per workgroup size over the ring pairs), then one launch of pg_fb_decode_trace over all pairs.
int pagan_fb_decode_batch(int32_t n, pagan_fb *const *fbs, double gap_weight, uint32_t flags, pagan_fb_decoded **out) {
    if (n < 0 || (flags & ~PAGAN_DECODE_KEEP_MATRIX) || !(gap_weight >= 0.0) || !(gap_weight < HUGE_VAL) || (n > 0 && (!fbs || !out))) return PAGAN_E_ARG;
    for (int k = 0; k < n; ++k) out[k] = nullptr;
    if (n == 0) return PAGAN_OK;
    FbCall c;
    FB_DO(c.open(n, fbs));
    // launch order: the fill pairs, then the ring pairs by workgroup size and by whether their score table needs looking at
    const FbSwitches sw = FbSwitches::read();
    std::vector<int> block(n, 0), order(n), tabfin(n, 1);
    for (int k = 0; k < n; ++k) {
        const pagan_fb *fb = fbs[k];
        if (fb_decode_route(fb->L, fb->R, fb->Lx, fb->Ly, fb->dx, sw)) block[k] = fb_block_for(fb->dx.max_width);
        for (float v : fb->score) if (!(v > 0.0f) || !(v < HUGE_VALF)) tabfin[k] = 0;
        order[k] = k;
    }
    auto launch_key = [&](int k) { return block[k] ? 2 * block[k] + (tabfin[k] ? 0 : 1) : 0; };
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return launch_key(a) < launch_key(b); });
    std::vector<std::unique_ptr<pagan_fb_decoded>> hs(n);
    FdStreamWait wait_on_exit;                                   // (declared behind the handles: runs before they are destroyed)
    const size_t o_jobs = c.take(FbCall::UP, (size_t)n * sizeof(PgFbJob)), o_recs = c.take(FbCall::UP, (size_t)n * sizeof(PgFbDecode));
    std::vector<size_t> o_sum(n), o_trace(n);
    for (int k = 0; k < n; ++k) o_sum[k] = c.take(FbCall::DOWN, fd_sizes(fbs[k]->dx.cells, fbs[k]->Lx, fbs[k]->Ly).summary);
    for (int k = 0; k < n; ++k) o_trace[k] = c.take(FbCall::DEVICE, fd_sizes(fbs[k]->dx.cells, fbs[k]->Lx, fbs[k]->Ly).trace);
    FB_DO(c.alloc());
    int fill_block = 64, n_fill = 0;
    for (int q = 0; q < n; ++q) {
        const int k = order[q];
        const pagan_fb *fb = fbs[k];
        hs[k].reset(new pagan_fb_decoded());
        pagan_fb_decoded *d = hs[k].get();
        d->bind(fb, 1, flags, c);
        d->schedule = block[k] ? 1 : 0;
        d->arena = slab_alloc(fb_arena_pool, d->device, fd_sizes(fb->dx.cells, fb->Lx, fb->Ly).matrix, &d->arena_cap);
        if (!d->arena) return PAGAN_E_NOMEM;
        if (flags & PAGAN_DECODE_KEEP_MATRIX) d->dx = fb->dx;
        d->d_trace = c.dev<const int>(o_trace[k]);
        PgFbDecode R;
        R.g = gap_weight; R.A = (double *)d->arena; R.trace = c.dev<int>(o_trace[k]); R.summary = c.dev<int>(o_sum[k]);
        R.max_steps = d->max_steps;
        R.tab_finite = tabfin[k];
        c.put(o_jobs + (size_t)q * sizeof(PgFbJob), fb->job);
        c.put(o_recs + (size_t)q * sizeof(PgFbDecode), R);
        if (!block[k]) { fill_block = std::max(fill_block, fb_block_for(fb->dx.max_width, true)); ++n_fill; }
    }
    const PgFbJob *jobs = c.dev<const PgFbJob>(o_jobs);
    const PgFbDecode *recs = c.dev<const PgFbDecode>(o_recs);
    FB_DO(c.upload());
    FB_DO(c.begin());
    for (int k = 0; k < n; ++k) { hs[k]->threads = block[k] ? block[k] : fill_block; hs[k]->tab = block[k] && !tabfin[k] ? 1 : 0; }
    if (n_fill > 0) hipLaunchKernelGGL(pg_fb_decode_fill, dim3((unsigned)n_fill), dim3((unsigned)fill_block), 0, nullptr, jobs, recs);
    for (int q = n_fill; q < n;) {
        const int b = block[order[q]], key = launch_key(order[q]);
        int e = q;
        while (e < n && launch_key(order[e]) == key) ++e;
        const dim3 grid((unsigned)(e - q)), blk((unsigned)b);
        if (b > 512 && tabfin[order[q]]) hipLaunchKernelGGL((pg_fb_ring_decode<1024, false>), grid, blk, 0, nullptr, jobs + q, recs + q);
        else if (b > 512) hipLaunchKernelGGL((pg_fb_ring_decode<1024, true>), grid, blk, 0, nullptr, jobs + q, recs + q);
        else if (tabfin[order[q]]) hipLaunchKernelGGL((pg_fb_ring_decode<512, false>), grid, blk, 0, nullptr, jobs + q, recs + q);
        else hipLaunchKernelGGL((pg_fb_ring_decode<512, true>), grid, blk, 0, nullptr, jobs + q, recs + q);
        q = e;
    }
    FB_DO(c.end());
    FB_DO(c.begin());
    hipLaunchKernelGGL(pg_fb_decode_trace, dim3((unsigned)n), dim3(64), 0, nullptr, jobs, recs);
    FB_DO(c.end());
    FB_DO(c.download());
    for (int k = 0; k < n; ++k) {
        pagan_fb_decoded *d = hs[k].get();
        d->keep_summary(c, o_sum[k]);
        if (k == 0) { d->ms[0] = c.ms(0); d->ms[1] = c.ms(1); }
        if (!(flags & PAGAN_DECODE_KEEP_MATRIX)) { give_slab(fb_arena_pool, d->device, d->arena, d->arena_cap); d->arena = nullptr; }
    }
    for (int k = 0; k < n; ++k) out[k] = hs[k].release();
    return PAGAN_OK;
}

int pagan_fb_decode(pagan_fb *fb, double gap_weight, uint32_t flags, pagan_fb_decoded **out) {
    if (!fb || !out) return PAGAN_E_ARG;
    return pagan_fb_decode_batch(1, &fb, gap_weight, flags, out);
}

int pagan_fb_decoded_summary(const pagan_fb_decoded *d, int32_t *status, double *objective, int32_t *n_steps, int32_t counts[3],
                             int32_t *schedule) {
    if (!d) return PAGAN_E_ARG;
    const int32_t *sm = d->sum(0);
    if (status) *status = sm[FB_SUM_STATUS];
    if (objective) *objective = d->value(0);
    if (n_steps) *n_steps = sm[FB_SUM_STEPS];
    if (counts) { counts[0] = sm[FB_SUM_M]; counts[1] = sm[FB_SUM_X]; counts[2] = sm[FB_SUM_Y]; }
    if (schedule) *schedule = d->schedule;
    return PAGAN_OK;
}

int pagan_fb_decoded_launch(const pagan_fb_decoded *d, int32_t *threads, int32_t *table_lookup) {
    if (!d) return PAGAN_E_ARG;
    if (threads) *threads = d->threads;
    if (table_lookup) *table_lookup = d->tab;
    return PAGAN_OK;
}

int pagan_fb_decoded_visited(pagan_fb_decoded *d, int32_t *visited, int32_t *n_visited) {
    if (!d || !visited) return PAGAN_E_ARG;
    return d->visited(0, visited, n_visited);
}

int pagan_fb_decoded_result(pagan_fb_decoded *d, pagan_result *out) {
    if (!d || !out) return PAGAN_E_ARG;
    return d->result(0, out);
}

// dst [Lx][Ly][3] row-major, state order X, Y, M; -inf outside the band
int pagan_fb_decoded_dump(pagan_fb_decoded *d, double *dst) {
    if (!d || !dst || !d->arena || !(d->flags & PAGAN_DECODE_KEEP_MATRIX)) return PAGAN_E_ARG;
    DeviceScope on_device(d->device);
    if (!on_device.ok) return PAGAN_E_NODEVICE;
    std::vector<double> a(3 * (size_t)d->cells);
    FB_TRY(hipMemcpy(a.data(), d->arena, 8 * a.size(), hipMemcpyDeviceToHost));
    for (int i = 0; i < d->Lx; ++i)
        for (int j = 0; j < d->Ly; ++j) {
            const long long at = d->dx.at(i, j);
            double *o = dst + ((size_t)i * d->Ly + j) * 3;
            for (int s = 0; s < 3; ++s) o[s] = at < 0 ? -HUGE_VAL : a[3 * at + s];
        }
    return PAGAN_OK;
}

int pagan_fb_decoded_ms(const pagan_fb_decoded *d, double ms[2]) {
    if (!d || !ms) return PAGAN_E_ARG;
    ms[0] = d->ms[0]; ms[1] = d->ms[1];
    return PAGAN_OK;
}

// What a decode takes beside the pair's own arena: A with the pool's allowance of a sixteenth (FbArenaPool::take), 12 B a path
// step, the summary and the records.
int64_t pagan_fb_decode_predict_bytes(int32_t left_sites, int32_t right_sites, const pagan_band *band) {
    const int64_t cells = pagan_dp_count_cells(left_sites, right_sites, band);
    if (cells < 0) return cells;
    const FdSizes z = fd_sizes(cells, left_sites - 1, right_sites - 1);
    return (int64_t)(z.matrix + z.matrix / 16 + z.trace + z.summary + sizeof(PgFbJob) + sizeof(PgFbDecode) + 1024);
}

void pagan_fb_decoded_destroy(pagan_fb_decoded *d) { delete d; }

} // extern "C"
