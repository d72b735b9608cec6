// dp_pipe_loader.inc -- the loader wave of pg_fill_pipe: site records, bwd edge lists and diagonal descriptors into the LDS
// windows ahead of the slowest compute wave (included by dp_pipe.hip, inside its anonymous namespace).
// ---- loader wave -------------------------------------------------------------------------
template <bool LEFT>
__device__ __forceinline__ void load_rec_chunk(int first, int lane, int n, gint_p st, gint_p off, gint_p src, gfloat_p lw, bool strip, bool norm,
                                               PG_GLOBAL const unsigned char *hf) {
    pg_i4 *rec = LEFT ? PM.recL : PM.recR;
    int *eb = LEFT ? PM.ebL : PM.ebR;
    int *es = LEFT ? PM.esL : PM.esR;
    float *ew = LEFT ? PM.ewL : PM.ewR;
    const int r = first + lane;
    // two round trips for the usual chunk: offsets and states, then the sites' first two edges together with the chunk's
    // edge list for the LDS window; a third (and on) only where a site has more than two edges
    int b = 0, en = 0, w = 0;
    unsigned flag = 0;                                             // far histories: the site's flag byte (0 where the job has none)
    if (r < n) { b = off[r]; en = off[r + 1]; w = st[r] & 0xffff; if (hf) flag = hf[r]; }
    const int ne = en - b;
    const int rend = first + 64 < n ? first + 64 : n;
    const int e0 = __builtin_amdgcn_readfirstlane(b), e1 = __builtin_amdgcn_readlane(en, rend - 1 - first);
    int d0 = 0, d1 = 0;
    float w0 = 0.0f, w1 = 0.0f;
    if (ne >= 1) { d0 = r - src[b]; w0 = lw[b]; }
    if (ne >= 2) { d1 = r - src[b + 1]; w1 = lw[b + 1]; }
    for (int e = e0 + lane; e < e1; e += 128) {
        const bool two = e + 64 < e1;
        const int s0 = src[e];
        const float x0 = lw[e];
        int s1 = 0;
        float x1 = 0.0f;
        if (two) { s1 = src[e + 64]; x1 = lw[e + 64]; }
        es[e & (PEC - 1)] = s0; ew[e & (PEC - 1)] = x0;
        if (two) { es[(e + 64) & (PEC - 1)] = s1; ew[(e + 64) & (PEC - 1)] = x1; }
    }
    if (r < n) {
        if (r > 0 && ne == 1 && d0 == 1 && w0 == 0.0f) w |= PR_SIMPLE;
        w |= (ne < 127 ? ne : 127) << PR_NE_SHIFT;
        if (norm && ne == 2 && (d0 == 1) != (d1 == 1)) {
            if (d0 != 1) { const int td = d0; d0 = d1; d1 = td; const float tw = w0; w0 = w1; w1 = tw; }
            w |= PR_TWO;
        }
        if (norm && ne == 3) {
            // three edges, exactly one from the previous site, none past the ring's reach (dp_abi.hip, SiteFeat::is_three -- the same
            // test): the site's list, in the record AND in the edge window, becomes (previous-site edge, other, other); values do not
            // depend on a list's order, and every reader of the window sees the same permuted list (this lane's LDS writes follow
            // the chunk's in the wave's order)
            int d2 = r - src[b + 2];
            float w2 = lw[b + 2];
            const int n_adj = (d0 == 1) + (d1 == 1) + (d2 == 1);
            const int far_ = d0 > d1 ? (d0 > d2 ? d0 : d2) : (d1 > d2 ? d1 : d2);
            if (n_adj == 1 && far_ <= PAGE - 2) {
                if (d1 == 1) { const int td = d0; d0 = d1; d1 = td; const float tw = w0; w0 = w1; w1 = tw; }
                else if (d2 == 1) { const int td = d0; d0 = d2; d2 = td; const float tw = w0; w0 = w2; w2 = tw; }
                es[b & (PEC - 1)] = r - d0; ew[b & (PEC - 1)] = w0;
                es[(b + 1) & (PEC - 1)] = r - d1; ew[(b + 1) & (PEC - 1)] = w1;
                es[(b + 2) & (PEC - 1)] = r - d2; ew[(b + 2) & (PEC - 1)] = w2;
                w |= PR_TWO | PR_THREE;
            }
        }
        pg_i4 v;
        v.x = w; v.y = (d0 < 65535 ? d0 : 65535) | ((d1 < 65535 ? d1 : 65535) << 16);
        v.z = __float_as_int(w0); v.w = __float_as_int(w1);
        // row strips: the first site (no bwd edge) is recorded as a SIMPLE one -- one edge of weight 1 from a site before it.
        // Whatever a cell of row 0 (column 0) reads of the row (column) before it is -inf (a ring column no wave writes, a lane
        // outside the band, a row outside the band for far_ask), which is what the general rules give its X and M (Y and M);
        // its y-gap (x-gap) chain is the straight code's at the terminal rate; the diagonals 0 and 1 and the cells that meet
        // M(0,0) through an edge from site 0 are general steps (dp_abi.hip, plan_strips), and those read no record of site 0.
        if (strip && r == 0) { v.x = (w & 0xffff) | PR_SIMPLE | (1 << PR_NE_SHIFT); v.y = 1; v.z = 0; v.w = 0; }
        // far histories (dp_abi.hip, plan_far_hist; flag byte: bit 7 reader + bits 0-1 its line, bit 6 writer + bits 4-5 its line)
        if (flag & 0x80u) v.x |= (int)(PR_FAR | ((flag & 3u) << 27));
        if (flag & 0x40u) v.x |= (int)(PR_SRC | (((flag >> 4) & 3u) << 25));
        rec[r & (PRW - 1)] = v;
        eb[r & (PRW - 1)] = b;
    }
}

// The site-record windows are filled as far ahead as they allow -- a record may replace the one PRW sites before it once
// the slowest wave's diagonal has left that site behind (a band's first row and first column never fall) -- and at least as
// far as the diagonal PLOOK ahead needs; the descriptor window follows PLOOK diagonals ahead.  One chunk of rows and one of
// columns per round, each published as it lands.
#define PREC_BACK 72              // 64 (a chunk) + 8: the records up to 8 sites before the slowest diagonal's first stay
// follow[0] = 1 + the last diagonal whose scores have landed in L2 (PgDevJob::follow; what the follower workgroups wait
// for): a wave's stores of diagonal d have landed once it completed d + PLAND; published every 16 diagonals or so
// (wt, row strips: written through -- the strip below may poll from another XCD)
__device__ __forceinline__ void publish_landed(PG_GLOBAL int *follow, int lane, int landed, bool wt = false) {
    if (follow && lane == 0) {
        if (wt) asm volatile("global_store_dword %0, %1, off sc1" :: "v"(follow), "v"(landed + 1) : "memory");
        else asm volatile("global_store_dword %0, %1, off" :: "v"(follow), "v"(landed + 1) : "memory");
    }
}
// Row strips (`strip`: the PgDevJob, null otherwise): records from the strip's first halo row / first column on, the
// descriptor window from the PARENT's array (whole-band rows per diagonal, offsets in cells there), everything from d_first.
__device__ __forceinline__ void pipe_loader(const View &J, cdesc8_p psc, int lane, PG_GLOBAL int *follow, const PgDevJob *strip, bool norm,
                                            PG_GLOBAL const unsigned char *hfl, PG_GLOBAL const unsigned char *hfr) {
    int rows = 0, cols = 0, diags = 0, published = -1;
    PG_GLOBAL const pg_i4 *pdsc = nullptr;
    if (strip) {
        rows = strip->strip_row0 >= 64 ? strip->strip_row0 - 64 : 0;
        cols = strip->col_first;
        diags = strip->d_first >= 64 ? strip->d_first - 64 : 0;
        published = strip->d_first - 1;
        pdsc = (PG_GLOBAL const pg_i4 *)strip->pdsc;
    }
    for (;;) {
        int pmin = flag_load(&PM.progress[0]);
        for (int w = 1; w < PNW; ++w) { const int p = flag_load(&PM.progress[w]); pmin = p < pmin ? p : pmin; }
        if (flag_load(&PM.abort_flag) != 0) { publish_landed(follow, lane, J.nd - 1, strip != nullptr); return; }   // (the job fails: the followers need not wait)
        // A compute wave's flag for the LAST diagonal goes up as after any other step -- with its stores still in flight -- so
        // the tail is published like the middle, PLAND behind the slowest wave, and the last diagonals only once every wave
        // has said "drained for good": progress = nd, stored behind the s_waitcnt vmcnt(0) that ends its last interval.
        if (pmin >= J.nd) { publish_landed(follow, lane, J.nd - 1, strip != nullptr); return; }
        if (pmin - PLAND >= published + (strip ? 8 : PG_FOLLOW_CHUNK)) { published = pmin - PLAND; publish_landed(follow, lane, published, strip != nullptr); }
        if (pmin + 1 >= J.nd) { __builtin_amdgcn_s_sleep(8); continue; }                          // nothing left to stage
        const int dcur = pmin + 1;                                 // the slowest wave may be computing this one
        const int da = dcur + PLOOK < J.nd - 1 ? dcur + PLOOK : J.nd - 1;
        const pg_i8 ds = psc[da], dc = psc[dcur];
        int want_rows = ds.y + 5, want_cols = da - ds.x + 4;       // rows <= hi+4, columns <= jmax+3 of diagonal da
        if (dc.y >= dc.x) {
            // as far ahead as the windows allow -- and no further: a record may only replace the one PRW sites before it, and those
            // of the slowest wave's diagonal (from PREC_BACK - 64 sites before its first row / column on) are still read.  (Round 5:
            // the look-ahead of PLOOK diagonals used to win over this bound; with diagonals of up to PG_PIPE_WINDOW cells it must not.)
            const int far_rows = dc.x + PRW - PREC_BACK, far_cols = dcur - dc.y + PRW - PREC_BACK;
            want_rows = far_rows;
            want_cols = far_cols;
            if (dc.y - dc.x + 1 > PG_PIPE_WINDOW) {
                // a diagonal wider than the windows (class 5) takes its records from L2, but its waves still wait for "rows <= hi + 3
                // loaded": just those, so that the first diagonal the windows cover again finds the records before its first row
                const pg_i8 dn = psc[dcur + 1 < J.nd ? dcur + 1 : dcur];
                const int near_rows = dn.y + 5, near_cols = dcur + 1 - dn.x + 4;
                want_rows = want_rows > near_rows ? want_rows : near_rows;
                want_cols = want_cols > near_cols ? want_cols : near_cols;
            }
        }
        want_rows = want_rows < J.Lx ? want_rows : J.Lx;
        want_cols = want_cols < J.Ly ? want_cols : J.Ly;
        bool any = false;
        // descriptors of the diagonals up to da: what a far read needs to find an old cell
        // (entries older than dcur - PDR + PLOOK are overwritten; readers look back PDR_REACH at most)
        if (diags <= da) {
            while (diags <= da) {
                const int t = diags + lane;
                if (t <= da) {
                    pg_i4 v;
                    if (pdsc) {
                        v = pdsc[t];
                        const long long bo = 24ll * (((long long)v.w << 32) | (unsigned)v.z);
                        v.z = (int)(bo & 0xffffffffLL); v.w = (int)(bo >> 32);
                    } else v = *((PG_GLOBAL const pg_i4 *)psc + 2 * t);
                    PM.dring[t & (PDR - 1)] = v;
                }
                diags = diags + 64 < da + 1 ? diags + 64 : da + 1;
            }
            flag_store(&PM.loaded[2], diags);
            any = true;
        }
        if (rows < want_rows) {
            load_rec_chunk<true>(rows, lane, J.Lx, J.stL, J.offL, J.srcL, J.lwL, strip != nullptr, norm, hfl);
            rows += 64; any = true;
            flag_store(&PM.loaded[0], rows);
        }
        if (cols < want_cols) {
            load_rec_chunk<false>(cols, lane, J.Ly, J.stR, J.offR, J.srcR, J.lwR, strip != nullptr, norm, hfr);
            cols += 64; any = true;
            flag_store(&PM.loaded[1], cols);
        }
        if (!any) __builtin_amdgcn_s_sleep(8);
    }
}
#undef PREC_BACK
