// dp_pipe_strip.inc -- what runs beside a fill workgroup's own waves: the follower workgroups (back-pointers behind the fill) and
// the feeder wave of a row strip (included by dp_pipe.hip, inside its anonymous namespace, in front of the kernel).
// ---------------------------------------------------------------------------------------------------------------------
// Follower workgroups (blockIdx.x >= n_fill of the same dispatch): back-pointers behind the fill.
//
// The fill stores scores only; the back-pointers are a function of the stored scores (pg_backptr, dp_kernels.hip) that needs
// no wave of the dependency chain.  A banded fill occupies 1 - 31 compute units for 45 - 170 ms, so the pass runs WHILE the
// fill goes on, on units it leaves idle: every wave of a follower workgroup claims chunks of PG_FOLLOW_CHUNK diagonals of a
// job (an atomic counter per job), waits until the scores of the chunk's predecessors have landed (follow[0], published by
// the job's loader wave) and writes the chunk's back-pointers.  The kernel ends a few microseconds after the last fill
// workgroup instead of being followed by a pass over every cell.
//
// Scores are read from L2 (sc1 loads: a line of the frontier may sit in this unit's L1 from an earlier diagonal).  L2 is per
// XCD: a follower serves only fill workgroups of its own XCD.  Workgroups of a dispatch go round the XCDs by index, so
// follower g looks at the jobs w with w % 8 == g % 8 and checks the XCC id the fill workgroup published; a job whose id
// differs, or never shows, is left alone.  Every wait is bounded; what no follower wrote (bp_done[chunk] == 0) pg_backptr
// writes after the kernel, so a follower that gives up costs time, not results.
__device__ __forceinline__ int peek_l2(PG_GLOBAL const int *p) {
    int v;
    asm volatile("global_load_dword %0, %1, off sc1\n\ts_waitcnt vmcnt(0)" : "=&v"(v) : "v"(p) : "memory");
    return __builtin_amdgcn_readfirstlane(v);
}
__device__ __forceinline__ unsigned my_xcc_id() {
    unsigned x;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(x));
    return x & 15u;
}

__device__ __noinline__ void follow_chunk(const PgDevJob *__restrict__ job, int chunk, int lane, unsigned flags) {
    const View J = load_view(job);
    const bool no_terminal_edges = flags & 1u;
    const bool reduced_terminal = !(flags & 2u);
    const int first = chunk * PG_FOLLOW_CHUNK, end = first + PG_FOLLOW_CHUNK < J.nd ? first + PG_FOLLOW_CHUNK : J.nd;
    for (int d = first; d < end; ++d) {
        const pg_i4 cur = J.dsc[d];
        const int lo = cur.x, hi = cur.y;
        if (hi < lo) continue;
        const long long base = ((long long)cur.w << 32) | (unsigned)cur.z;
        Diag d1 = {0, -1, 0}, d2 = {0, -1, 0};
        if (d > 0) { const pg_i4 p = J.dsc[d - 1]; d1 = {p.x, p.y, ((long long)p.w << 32) | (unsigned)p.z}; }
        if (d > 1) { const pg_i4 p = J.dsc[d - 2]; d2 = {p.x, p.y, ((long long)p.w << 32) | (unsigned)p.z}; }
        for (int i = lo + lane; i <= hi; i += 64) {
            const int j = d - i;
            const long long at = base + (i - lo);
            int l0 = 0, l1 = 0, r0 = 0, r1 = 0;
            if (i > 0) { l0 = J.offL[i]; l1 = J.offL[i + 1]; }
            if (j > 0) { r0 = J.offR[j]; r1 = J.offR[j + 1]; }
            float sm = 0.0f;
            if (i > 0 && j > 0 && l1 > l0 && r1 > r0) sm = J.table[J.stL[i] + J.stR[j] * J.S];       // VA:1363
            double bx, by, bm;
            unsigned px, py, pm;
            cell_any(J, i, j, l1 - l0, r1 - r0, sm, no_terminal_edges, reduced_terminal,
                     [&](int p, int q, double &xs, double &ys, double &ms) {
                         const long long ix = hbm_index(J, d, d1, d2, p, q);
                         xs = ys = ms = neg_inf();
                         if (ix >= 0) far_cell((PG_GLOBAL const double *)(J.sc + 3 * ix), xs, ys, ms);
                     },
                     [&](int k, int &p, double &lw) { p = J.srcL[l0 + k]; lw = (double)J.lwL[l0 + k]; },
                     [&](int k, int &q, double &rw) { q = J.srcR[r0 + k]; rw = (double)J.lwR[r0 + k]; },
                     bx, by, bm, px, py, pm);
            typedef unsigned u3 __attribute__((ext_vector_type(3)));
            u3 b; b.x = px; b.y = py; b.z = pm;
            *(PG_GLOBAL u3 *)(J.bp + 3 * at) = b;
            if (flags & PG_FLAG_SCORE_CHECK) {
                // the recurrence holds at this cell, bit for bit (dp_kernels.hip, pg_backptr has the reasoning): the cell's own
                // scores have landed with its diagonal (the chunk is claimed behind the landed counter)
                double sx, sy, sm_;
                far_cell((PG_GLOBAL const double *)(J.sc + 3 * at), sx, sy, sm_);
                const bool same = __double_as_longlong(bx) == __double_as_longlong(sx) && __double_as_longlong(by) == __double_as_longlong(sy) &&
                                  __double_as_longlong(bm) == __double_as_longlong(sm_);
                if (!same) report_fill_status(job, PG_FILL_SCORE_MISMATCH);
            }
        }
    }
    if (lane == 0) ((PG_GLOBAL unsigned char *)job->bp_done)[chunk] = 1;
}

__device__ __noinline__ void pipe_follower(const PgDevJob *__restrict__ jobs, const int *__restrict__ which, int n_fill, unsigned flags) {
    const int lane = threadIdx.x & 63;
    const unsigned xcc = my_xcc_id();
    // the jobs of this dispatch whose fill workgroup runs on this XCD (at most four: 31 jobs a dispatch)
    int mine[4], n_mine = 0;
    for (int w = (int)(blockIdx.x & 7u); w < n_fill && n_mine < 4; w += 8) {
        const PgDevJob *__restrict__ job = jobs + which[w];
        if (!job->follow) continue;
        int id = 0;
        for (int spin = 0; spin < 20000 && (id = peek_l2((PG_GLOBAL const int *)job->follow + 1)) == 0; ++spin) __builtin_amdgcn_s_sleep(32);
        if (id == (int)xcc + 1) mine[n_mine++] = which[w];
    }
    unsigned left = (1u << n_mine) - 1u;
    int idle = 0;
    const int start = (int)(threadIdx.x >> 6);                    // the waves of a workgroup start at different jobs
    while (left != 0 && idle < 200000) {
        bool worked = false;
        for (int t = 0; t < n_mine; ++t) {
            const int k = (t + start) % n_mine;
            if (!(left & (1u << k))) continue;
            const PgDevJob *__restrict__ job = jobs + mine[k];
            PG_GLOBAL int *fw = (PG_GLOBAL int *)job->follow;
            const int nd = job->nd, n_chunks = (nd + PG_FOLLOW_CHUNK - 1) / PG_FOLLOW_CHUNK;
            const int next = peek_l2(fw + 2);
            if (next >= n_chunks) { left &= ~(1u << k); continue; }
            // a chunk's cells read the diagonals below its last one: claim it once those have landed
            // (with the score check the chunk's own last diagonal is read too: one more)
            const int chk = (flags & PG_FLAG_SCORE_CHECK) ? 1 : 0;
            const int last = ((next + 1) * PG_FOLLOW_CHUNK - 1 < nd - 1 ? (next + 1) * PG_FOLLOW_CHUNK - 1 : nd - 1) + chk;
            if (peek_l2(fw) < last) continue;                      // (follow[0] = landed + 1 >= last: diagonals <= last - 1 are there)
            int c = 0;
            if (lane == 0) c = __hip_atomic_fetch_add(fw + 2, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            c = __builtin_amdgcn_readfirstlane(c);
            if (c >= n_chunks) { left &= ~(1u << k); continue; }
            // (another wave may have taken `next` in between: c is a later chunk, wait for it)
            const int lastc = ((c + 1) * PG_FOLLOW_CHUNK - 1 < nd - 1 ? (c + 1) * PG_FOLLOW_CHUNK - 1 : nd - 1) + chk;
            int spin = 0;
            while (peek_l2(fw) < lastc && spin < 200000) { __builtin_amdgcn_s_sleep(32); ++spin; }
            if (spin >= 200000) return;                            // the fill stopped publishing: pg_backptr writes this chunk
            follow_chunk(job, c, lane, flags);
            worked = true;
        }
        if (worked) idle = 0; else { __builtin_amdgcn_s_sleep(64); ++idle; }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// Row strips: a wide job (a full matrix, a band wider than the lanes) as a chain of banded jobs.
//
// A strip is PG_STRIP_ROWS = 192 rows of the matrix over all their columns: to this kernel a band whose first and last
// row stand still.  Rows map to lanes as ever (row % 256), so a strip's rows fill three compute waves; the fourth -- the
// wave "upstream" of the strip's first row -- is its FEEDER: it owns the 64 rows above the strip, computes nothing, and
// writes the cells of the last PHALO = 16 of them (a ring operand lies at most PAGE - 1 rows up; the other columns stay
// -inf and are never read), read back from the scores the strip above stored, into its ring columns diagonal by diagonal,
// publishing its progress like any compute wave.  To the strip's waves the rows above are in the ring exactly as if a
// wave had computed them: lane 0 of the first wave takes row-1 from the feeder's lane 63 (the hot loop checks the feeder's
// flag as it checks any upstream wave's), multi-edge cells find their ring operands above the strip in the ring, and ring
// rows are reused under the same per-diagonal rule.  A strip starts when the one above has landed the diagonals its first
// cells read, and then follows it a few dozen diagonals behind: the job's anti-diagonal sweeps all its strips at once.
// Strip -> strip visibility (round 5): a strip's scores and its "landed" counter are written THROUGH to memory (sc1 stores:
// store_scores, the strips' assembly loop, publish_landed) and read with sc1 loads (far_fetch*, peek_l2), so the strips of a
// job run on whatever XCD the dispatcher gives them -- HIP promises no placement.  Round 4's form is behind
// PAGAN_DP_STRIP_SPREAD=0: a job's strips at workgroup indices of one residue mod 8 (one XCD as dispatches are observed to
// go), each strip publishing its XCC id and the feeder below checking it (tag 11; the host's re-runs: dp_abi.hip).
#define PHALO 16                  // rows above the strip the feeder keeps in the ring: a ring operand lies at most PAGE - 1 <= 16 rows up
#define PFEED 32                  // diagonals the feeder requests from L2 at a time: 4 per load (lane = diagonal % 4, row), 8 loads, one round trip
static_assert(PHALO >= PAGE - 1 && 64 / PHALO * 8 == PFEED, "feeder geometry");
__device__ __noinline__ void strip_feeder(const PgDevJob *__restrict__ job, cdesc8_p psc, int tid, int wave, unsigned flags) {
    const int lane = tid & 63;
    wave = __builtin_amdgcn_readfirstlane(wave);
    const int nd = job->nd, d0 = job->d_first;
    const int hq = lane / PHALO, hr = lane % PHALO;                // this lane's diagonal (of four) and halo row in a request
    const int row = job->strip_row0 - PHALO + hr;
    const int col = row & (PNT - 1);                               // its ring column (the last PHALO lanes' of this wave)
    const int dn = (wave + 1) % PNW;
    PG_GLOBAL const int *prev = (PG_GLOBAL const int *)job->prev_follow;
    const int prev_last = job->prev_nd - 1;
    PG_GLOBAL const pg_i4 *pdsc = (PG_GLOBAL const pg_i4 *)job->pdsc;
    const gdouble_w sc = (gdouble_w)job->sc;
    const double NI = neg_inf();
    int d = d0;                                                    // (names the diagonal in an abort tag)
    flag_store(&PM.arrived[wave], nd);                             // no stores to drain: never what a rendezvous waits for
    if (!(flags & PG_FLAG_STRIPS_SPREAD)) {
        // PAGAN_DP_STRIP_SPREAD=0 (round 4's placement): the strip above runs on this XCD
        int id = 0, spin = 0;
        while ((id = peek_l2(prev + 1)) == 0 && spin < (1 << 22) && flag_load(&PM.abort_flag) == 0) { __builtin_amdgcn_s_sleep(16); ++spin; }
        // (debug flag 0x800, tests: as if it did not -- the host clears the bit when it launches the strips alone)
        if ((id != (int)my_xcc_id() + 1 || (flags & 0x800u)) && flag_load(&PM.abort_flag) == 0) flag_store(&PM.abort_flag, PTAG(11));
    }
    int landed1 = 0, p_dn = d0 - 1, slot = d0 % PRK;
    for (int t0 = d0; t0 < nd && flag_load(&PM.abort_flag) == 0; t0 += PFEED) {
        const int t1 = t0 + PFEED < nd ? t0 + PFEED : nd;
        d = t0;
        // what the strip above stored of the diagonals t0 .. t1-1 has landed (its counter ends at its own last diagonal)
        const int need1 = (t1 - 1 < prev_last ? t1 - 1 : prev_last) + 1;
        if (landed1 < need1) {
            int spin = 0;
            while ((landed1 = peek_l2(prev)) < need1) {
                __builtin_amdgcn_s_sleep(4);
                if (++spin > PSPIN_LIMIT / 8 || flag_load(&PM.abort_flag) != 0) {
                    if (flag_load(&PM.abort_flag) == 0) flag_store(&PM.abort_flag, PTAG(12));
                    break;
                }
            }
            if (landed1 < need1) break;
        }
        FarAsk fa[8];
        pg_d2 xy[8];
        double m[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {                              // request k: the diagonals t0 + 4k .. t0 + 4k + 3, this lane's t0 + 4k + hq
            const int t = t0 + 4 * k + hq;
            const pg_i4 ds = pdsc[t < nd ? t : nd - 1];            // the whole band's rows on t, the offset (in cells) of its first
            fa[k].need = t < t1 && row >= ds.x && row <= ds.y;
            fa[k].boff = 24ll * ((((long long)ds.w << 32) | (unsigned)ds.z) + (row - ds.x));
            xy[k].x = NI; xy[k].y = NI; m[k] = NI;
        }
        // the batch's ring-reuse rule (descriptor word 7: what the downstream wave must have completed, as for any wave) in one load
        const int s7v = ((PG_GLOBAL const int *)psc)[8 * (t0 + (lane & 31) < nd ? t0 + (lane & 31) : nd - 1) + 7];
        far_fetch8(sc, fa, xy, m);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
#pragma unroll
            for (int q = 0; q < 64 / PHALO; ++q) {
                const int t = t0 + 4 * k + q;
                if (t >= t1) break;
                d = t;
                const int s7 = __builtin_amdgcn_readlane(s7v, 4 * k + q);
                if (s7 > p_dn) p_dn = poll_ge(&PM.progress[dn], s7, PTAG(3));
                if (hq == q) { PM.sc[slot][col][PG_X] = xy[k].x; PM.sc[slot][col][PG_Y] = xy[k].y; PM.sc[slot][col][PG_M] = m[k]; }
                flag_store_inorder(&PM.progress[wave], t);          // (behind the cell: a wave's LDS operations execute in order)
                slot = slot + 1 == PRK ? 0 : slot + 1;
            }
        }
    }
    flag_store(&PM.progress[wave], nd);
}
#undef PHALO
#undef PFEED
