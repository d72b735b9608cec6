// dp_anc_nni.inc -- tree search by nearest-neighbour interchange (include/pagan_host.h, "tree search by nearest-neighbour
// interchange"; DESIGN.md "Tree search by nearest-neighbour interchange"), included at the end of dp_anc.hip behind
// dp_anc_brlen.inc: pa_encode, pa_up and pa_down are launched as they are, and the run is BrlenRun with a tree that changes.
// After the two passes every candidate edge is independent of every other, so nothing here walks the node schedule and nothing
// is handed from one workgroup to another: no flags, no counters, no atomics.
//   pa_nni        a workgroup a (block of 64 columns, candidate); a lane a column.  The messages of a, d and b (and of e at the
//                 root edge: a decision the whole workgroup reads from the candidate table) come from pa_message as it stands.
//                 u_0 = m_a m_d, u_1 = m_b m_d, u_2 = m_a m_b; y_k = P_mid u_k for the three k in one sweep over P_mid;
//                 f_k = sum_s (T[s] X_k[s]) y_k[s].  S = 4 runs in registers on one wave; for S = 20 and 61 the four waves split
//                 the states as pa_down's do: the three u_k go through LDS (three S x 64 buffers) behind a __syncthreads, and the
//                 terms (T X_k) y_k through the same buffers to wave 0, which adds them in state order.  Then the ratios, frexp and
//                 the header's tree over the 64 columns (a shuffle a step); lane 0 stores the block's (m, e) and the degenerate
//                 counts of both arrangements.
//   pa_nni_fold   a thread a candidate multiplies the blocks in index order onto the running pairs, which survive from chunk to
//                 chunk.  The blocks' results are kept [block][field][candidate], so a wave's loads are contiguous.
// P (kept [t][s]) and the candidate table are __restrict__ parameters that are never stored to, so their loads stay scalar loads.

namespace pagan {

namespace {

struct NniArgs {
    double *block_m;                 // [C / 64][2][nc]
    int32_t *block_e;                // [C / 64][4][nc]: e of arrangement 1, 2, degenerate columns of 1, 2
    uint32_t nc;                     // the table's slots: n - 1
    uint32_t ncand;                  // the candidates listed in slots 0 .. ncand-1
    uint32_t cols;                   // the chunk's columns that are the alignment's
};

template <int S, int W>
__global__ __launch_bounds__(64 * W) void pa_nni(AncArgs A, NniArgs N, const double *__restrict__ PT, const double *__restrict__ pi, const int32_t *__restrict__ cand,
                                                const unsigned char *__restrict__ codes) {
    const AncModel M{nullptr, PT, pi, nullptr, codes};
    constexpr int NS = (S + W - 1) / W;
    __shared__ double xu[W > 1 ? 3 * S * 64 : 1];
    const uint32_t lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), s0 = wave * NS;
    const uint32_t block = blockIdx.x / N.ncand, j = blockIdx.x % N.ncand, nc = N.nc;
    const uint64_t col = (uint64_t)block * 64 + lane;
    const int32_t a = cand[j], d = cand[nc + j], b = cand[2 * nc + j], e = cand[3 * nc + j];
    const int32_t ma = cand[4 * nc + j], md = cand[5 * nc + j], mb = cand[6 * nc + j], me = cand[7 * nc + j], mid = cand[8 * nc + j], kv = cand[9 * nc + j];
    double xa[NS], xd[NS], xb[NS], T[NS];
    bool has, ha, hd, hb;
    pa_message<S, NS>(A, M, a, ma, s0, col, xa, ha);
    pa_message<S, NS>(A, M, d, md, s0, col, xd, hd);
    pa_message<S, NS>(A, M, b, mb, s0, col, xb, hb);
    if (e >= 0) {                                      // (the same in every thread of the workgroup) the root edge: T = pi m_e
        pa_message<S, NS>(A, M, e, me, s0, col, T, has);
#pragma unroll
        for (int q = 0; q < NS; ++q) T[q] = s0 + q < (uint32_t)S ? pi[s0 + q] * T[q] : 0.0;
    } else {
#pragma unroll
        for (int q = 0; q < NS; ++q) T[q] = s0 + q < (uint32_t)S ? A.outs[((uint64_t)kv * S + s0 + q) * A.C + col] : 0.0;
    }
    double y0[NS], y1[NS], y2[NS];
#pragma unroll
    for (int q = 0; q < NS; ++q) y0[q] = y1[q] = y2[q] = 0.0;
    const double *Pm = PT + (uint64_t)mid * S * S + s0;             // P_mid[s0 + q][t] at Pm[t * S + q]
    double f0 = 0.0, f1 = 0.0, f2 = 0.0;
    if constexpr (W > 1) {
#pragma unroll
        for (int q = 0; q < NS; ++q)
            if (s0 + q < (uint32_t)S) {
                xu[(s0 + q) * 64 + lane] = xa[q] * xd[q];
                xu[(S + s0 + q) * 64 + lane] = xb[q] * xd[q];
                xu[(2 * S + s0 + q) * 64 + lane] = xa[q] * xb[q];
            }
        __syncthreads();
#pragma unroll 2
        for (int t = 0; t < S; ++t) {
            const double u0 = xu[t * 64 + lane], u1 = xu[(S + t) * 64 + lane], u2 = xu[(2 * S + t) * 64 + lane];
#pragma unroll
            for (int q = 0; q < NS; ++q)
                if (s0 + q < (uint32_t)S) {
                    const double p = Pm[t * S + q];
                    y0[q] += p * u0;
                    y1[q] += p * u1;
                    y2[q] += p * u2;
                }
        }
        __syncthreads();                               // every wave has read the u_k
#pragma unroll
        for (int q = 0; q < NS; ++q) {                 // a pair without data is a node without data: the exact 1, as in the up pass
            if (!(ha || hd)) y0[q] = 1.0;
            if (!(hb || hd)) y1[q] = 1.0;
            if (!(ha || hb)) y2[q] = 1.0;
        }
#pragma unroll
        for (int q = 0; q < NS; ++q)
            if (s0 + q < (uint32_t)S) {
                xu[(s0 + q) * 64 + lane] = (T[q] * xb[q]) * y0[q];
                xu[(S + s0 + q) * 64 + lane] = (T[q] * xa[q]) * y1[q];
                xu[(2 * S + s0 + q) * 64 + lane] = (T[q] * xd[q]) * y2[q];
            }
        __syncthreads();
        if (wave != 0) return;                         // (after the last barrier)
        for (int s = 0; s < S; ++s) {
            f0 += xu[s * 64 + lane];
            f1 += xu[(S + s) * 64 + lane];
            f2 += xu[(2 * S + s) * 64 + lane];
        }
    } else {
        double u0[NS], u1[NS], u2[NS];
#pragma unroll
        for (int q = 0; q < NS; ++q) { u0[q] = xa[q] * xd[q]; u1[q] = xb[q] * xd[q]; u2[q] = xa[q] * xb[q]; }
#pragma unroll
        for (int t = 0; t < NS; ++t)
#pragma unroll
            for (int q = 0; q < NS; ++q) {
                const double p = Pm[t * S + q];
                y0[q] += p * u0[t];
                y1[q] += p * u1[t];
                y2[q] += p * u2[t];
            }
#pragma unroll
        for (int q = 0; q < NS; ++q) {                 // a pair without data is a node without data: the exact 1, as in the up pass
            if (!(ha || hd)) y0[q] = 1.0;
            if (!(hb || hd)) y1[q] = 1.0;
            if (!(ha || hb)) y2[q] = 1.0;
        }
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            f0 += (T[s] * xb[s]) * y0[s];
            f1 += (T[s] * xa[s]) * y1[s];
            f2 += (T[s] * xd[s]) * y2[s];
        }
    }
    const bool live = col < N.cols;
    double m[2];
    int ex[2], count[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const double fk = k ? f2 : f1;
        const bool good = f0 > 0.0 && fk > 0.0;
        const double r = live && good ? fk / f0 : 1.0;
        count[k] = __popcll(__ballot(live && !good));
        int ek = 0;
        double mk = frexp(r, &ek);
#pragma unroll
        for (int dd = 32; dd >= 1; dd >>= 1) {        // the header's tree: lane i < dd takes lane i + dd's pair
            const double mo = __shfl_down(mk, dd, 64);
            const int eo = __shfl_down(ek, dd, 64);
            int de = 0;
            mk = frexp(mk * mo, &de);
            ek = ek + eo + de;
        }
        m[k] = mk; ex[k] = ek;
    }
    if (lane == 0) {
        N.block_m[((uint64_t)block * 2 + 0) * nc + j] = m[0];
        N.block_m[((uint64_t)block * 2 + 1) * nc + j] = m[1];
        int32_t *to = N.block_e + (uint64_t)block * 4 * nc + j;
        to[0] = ex[0]; to[nc] = ex[1]; to[2 * nc] = count[0]; to[3 * nc] = count[1];
    }
}

__global__ __launch_bounds__(64) void pa_nni_fold(const double *__restrict__ block_m, const int32_t *__restrict__ block_e, double *run_m, long long *run_e, uint32_t nc,
                                                 uint32_t ncand, uint32_t blocks) {
    const uint32_t j = blockIdx.x * 64 + threadIdx.x;
    if (j >= ncand) return;
    for (int k = 0; k < 2; ++k) {
        double Mk = run_m[(uint64_t)k * nc + j];
        long long Ek = run_e[(uint64_t)k * nc + j], deg = run_e[(uint64_t)(2 + k) * nc + j];
        for (uint32_t q = 0; q < blocks; ++q) {
            int de = 0;
            Mk = frexp(Mk * block_m[((uint64_t)q * 2 + k) * nc + j], &de);
            Ek = Ek + block_e[((uint64_t)q * 4 + k) * nc + j] + de;
            deg += block_e[((uint64_t)q * 4 + 2 + k) * nc + j];
        }
        run_m[(uint64_t)k * nc + j] = Mk;
        run_e[(uint64_t)k * nc + j] = Ek; run_e[(uint64_t)(2 + k) * nc + j] = deg;
    }
}

template <int S, int W>
void launch_nni(const AncArgs &A, const NniArgs &N, const AncModel &M, const int32_t *cand, hipStream_t st) {
    hipLaunchKernelGGL((pa_nni<S, W>), dim3(A.C / 64 * N.ncand), dim3(64 * W), 0, st, A, N, M.PT, M.pi, cand, M.codes);
}

// One call's device state with a tree that changes: BrlenRun's buffers and passes, the candidate table, the running pairs.
struct NniRun {
    DevBuf own;                      // the candidate table, the blocks' pairs, the running pairs (before R: freed after R's stream has drained)
    BrlenRun R;
    AncNniLayout nl{2, 64};
    std::vector<int32_t> left, right, kind, cand;
    std::vector<double> branch;
    int ncand = 0;
    bool fresh = false;              // the partials on the device are those of this tree at these lengths (one chunk)
    double nni_ms = 0.0, fold_ms = 0.0;
    int rounds = 0;

    int setup(int32_t n, const int32_t *left_, const int32_t *right_, const double *branch_, const char *const *rows, int32_t data_type, const float *base_freq);
    int set_tree(const std::vector<int32_t> &l, const std::vector<int32_t> &r, const std::vector<double> &br);
    int up(double *ll);
    int gains(double *ll, double *M, int64_t *E, double *gain, int64_t *degenerate);
    void fill(pagan_anc_nni_info *info) const;
};

int NniRun::setup(int32_t n, const int32_t *left_, const int32_t *right_, const double *branch_, const char *const *rows, int32_t data_type, const float *base_freq) {
    R.extra_matrices = 1;            // the root edge's P_mid
    int rc = R.setup(n, left_, right_, branch_, rows, data_type, base_freq);
    if (rc != PAGAN_OK) return rc;
    nl = AncNniLayout(n, R.C);
    HIPA(own.alloc(nl.total));
    R.info.device_bytes += (int64_t)nl.total;
    return set_tree(std::vector<int32_t>(left_, left_ + n - 1), std::vector<int32_t>(right_, right_ + n - 1), std::vector<double>(branch_, branch_ + 2 * n - 1));
}

// the node table, the matrices and the candidate table of this tree at these lengths; the stream is idle on entry and on return
int NniRun::set_tree(const std::vector<int32_t> &l, const std::vector<int32_t> &r, const std::vector<double> &br) {
    left = l; right = r; branch = br;
    const int n = R.n, in = R.in, nb = R.nb;
    kind.assign((size_t)in, 0);
    std::vector<int32_t> parent((size_t)2 * n - 1, -1);
    nni_kinds(n, left.data(), right.data(), kind.data(), parent.data());
    R.set_tree(left.data(), right.data());
    const int32_t rl = left[in - 1], rr = right[in - 1];
    int rc = R.set_lengths(branch.data());
    if (rc != PAGAN_OK) return rc;
    // P_mid of the root edge: one more matrix behind those of the distinct lengths, both ways round as they are
    const size_t SS = (size_t)R.S * R.S;
    const int mid_matrix = (int)(R.P.size() / SS);
    std::vector<double> pm(SS), pmt(SS);
    if (rl >= n && kind[rl - n] == 2) {
        anc_pmatrix(R.mf, branch[rl] + branch[rr], pm.data());
        for (int s = 0; s < R.S; ++s) for (int t = 0; t < R.S; ++t) pmt[(size_t)t * R.S + s] = pm[(size_t)s * R.S + t];
        HIPA(hipMemcpyAsync(R.base + R.lay.P + mid_matrix * SS * sizeof(double), pm.data(), SS * sizeof(double), hipMemcpyHostToDevice, R.D.st));
        HIPA(hipMemcpyAsync(R.base + R.lay.PT + mid_matrix * SS * sizeof(double), pmt.data(), SS * sizeof(double), hipMemcpyHostToDevice, R.D.st));
    }
    cand.assign((size_t)kNniCandFields * in, -1);
    ncand = 0;
    auto matrix = [&](int32_t v) { return R.branches[(size_t)3 * nb + v]; };
    for (int q = 0; q < in; ++q) {
        if (!kind[q]) continue;
        const int32_t c = n + q, a = left[q], d = right[q];
        int32_t b, e = -1, mid, kv;
        if (kind[q] == 1) {
            const int32_t v = parent[c];
            b = left[v - n] == c ? right[v - n] : left[v - n];
            mid = matrix(c); kv = v - n;
        } else {
            e = left[rr - n]; b = right[rr - n];
            mid = mid_matrix; kv = -1;
        }
        const int32_t row[kNniCandFields] = {a, d, b, e, matrix(a), matrix(d), matrix(b), e >= 0 ? matrix(e) : 0, mid, kv, c};
        for (int f = 0; f < kNniCandFields; ++f) cand[(size_t)f * in + ncand] = row[f];
        ++ncand;
    }
    HIPA(hipMemcpyAsync(own.h + nl.cand, cand.data(), cand.size() * sizeof(int32_t), hipMemcpyHostToDevice, R.D.st));
    HIPA(hipStreamSynchronize(R.D.st));
    fresh = false;
    return PAGAN_OK;
}

int NniRun::up(double *ll) {
    const int rc = R.pass(BrlenRun::UP_ONLY, ll);
    fresh = rc == PAGAN_OK && R.chunks == 1;
    return rc;
}

// the down pass (the up pass before it where the partials are not this tree's), pa_nni, pa_nni_fold; outputs by internal node
int NniRun::gains(double *ll, double *M_out, int64_t *E_out, double *gain_out, int64_t *deg_out) {
    const int n = R.n, in = R.in, S = R.S;
    const int64_t C = R.C;
    char *base = R.base, *mine = own.h;
    hipStream_t st = R.D.st;
    const bool with_up = !fresh;
    AncArgs A;
    AncModel M;
    BranchArgs B{nullptr, nullptr, (uint32_t)R.nb};
    NniArgs N;
    A.part = (double *)(base + R.lay.part); A.outs = (double *)(base + R.lay.outs);
    A.col_lik = (double *)(base + R.lay.col_lik); A.col_exp = (int32_t *)(base + R.lay.col_exp);
    A.best = (unsigned char *)(base + R.lay.best); A.best_p = (float *)(base + R.lay.best_p); A.post = nullptr;
    A.n = n; A.C = (uint32_t)C;
    M.P = (double *)(base + R.lay.P); M.PT = (double *)(base + R.lay.PT); M.pi = (double *)(base + R.lay.pi); M.nodes = (int32_t *)(base + R.lay.nodes);
    N.block_m = (double *)(mine + nl.block_m); N.block_e = (int32_t *)(mine + nl.block_e);
    N.nc = (uint32_t)in; N.ncand = (uint32_t)ncand;
    double *run_m = (double *)(mine + nl.run_m);
    long long *run_e = (long long *)(mine + nl.run_e);
    const int32_t *d_cand = (const int32_t *)(mine + nl.cand);
    if ((uint64_t)(C / 64) * (uint64_t)std::max(ncand, 1) > 0x7fffffffull) return PAGAN_E_ARG;       // pa_nni's grid
    std::vector<double> m0((size_t)2 * in, 0.5);
    std::vector<long long> e0((size_t)4 * in, 0);
    std::fill(e0.begin(), e0.begin() + (size_t)2 * in, 1);
    HIPA(hipMemcpyAsync(run_m, m0.data(), m0.size() * sizeof(double), hipMemcpyHostToDevice, st));
    HIPA(hipMemcpyAsync(run_e, e0.data(), e0.size() * sizeof(long long), hipMemcpyHostToDevice, st));
    auto stage = [&](int which) {
        if (S == 4) launch_stage<4, 1>(which, A, M, B, nullptr, nullptr, nullptr, st);
        else if (S == 20) launch_stage<20, 4>(which, A, M, B, nullptr, nullptr, nullptr, st);
        else launch_stage<61, 4>(which, A, M, B, nullptr, nullptr, nullptr, st);
    };
    const double ln2 = std::log(2.0);
    double total = 0.0;
    hipEvent_t ev[5] = {R.D.ev[0], R.D.ev[1], R.D.ev[2], R.D.ev[3], R.more[0]};
    for (int64_t ch = 0; ch < R.chunks; ++ch) {
        const int64_t c0 = ch * C, cols = std::max<int64_t>(0, std::min(C, R.L - c0));
        A.has = (unsigned char *)(base + R.lay.has) + (size_t)ch * (2 * n - 1) * C;
        M.codes = (unsigned char *)(base + R.lay.codes) + (size_t)ch * n * C;
        N.cols = (uint32_t)cols;
        HIPA(hipEventRecord(ev[0], st));
        if (with_up) stage(0);
        HIPA(hipEventRecord(ev[1], st));
        stage(1);
        HIPA(hipEventRecord(ev[2], st));
        if (ncand > 0) {
            if (S == 4) launch_nni<4, 1>(A, N, M, d_cand, st);
            else if (S == 20) launch_nni<20, 4>(A, N, M, d_cand, st);
            else launch_nni<61, 4>(A, N, M, d_cand, st);
        }
        HIPA(hipEventRecord(ev[3], st));
        if (ncand > 0) hipLaunchKernelGGL(pa_nni_fold, dim3((ncand + 63) / 64), dim3(64), 0, st, N.block_m, N.block_e, run_m, run_e, N.nc, N.ncand, (uint32_t)(C / 64));
        HIPA(hipEventRecord(ev[4], st));
        HIPA(hipGetLastError());
        if (with_up) {
            HIPA(hipMemcpyAsync(R.lik.data(), A.col_lik, (size_t)cols * sizeof(double), hipMemcpyDeviceToHost, st));
            HIPA(hipMemcpyAsync(R.expo.data(), A.col_exp, (size_t)cols * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        }
        HIPA(hipStreamSynchronize(st));
        float ms[4] = {0, 0, 0, 0};
        for (int e = 0; e < 4; ++e) HIPA(hipEventElapsedTime(&ms[e], ev[e], ev[e + 1]));
        R.info.up_ms += ms[0]; R.info.down_ms += ms[1]; nni_ms += ms[2]; fold_ms += ms[3];
        if (with_up)
            for (int64_t c = 0; c < cols; ++c) total += std::log(R.lik[c]) + R.expo[c] * ln2;       // (pagan_anc_reconstruct's sum)
    }
    if (with_up) { ++R.info.up_passes; if (ll) *ll = total; fresh = R.chunks == 1; }
    ++rounds;
    HIPA(hipMemcpy(m0.data(), run_m, m0.size() * sizeof(double), hipMemcpyDeviceToHost));
    HIPA(hipMemcpy(e0.data(), run_e, e0.size() * sizeof(long long), hipMemcpyDeviceToHost));
    for (int q = 0; q < 2 * in; ++q) {
        if (M_out) M_out[q] = 0.5;
        if (E_out) E_out[q] = 1;
        if (gain_out) gain_out[q] = 0.0;
        if (deg_out) deg_out[q] = 0;
    }
    for (int j = 0; j < ncand; ++j) {
        const int q = cand[(size_t)10 * in + j] - n;
        for (int k = 0; k < 2; ++k) {
            const double Mk = m0[(size_t)k * in + j];
            const long long Ek = e0[(size_t)k * in + j];
            if (M_out) M_out[2 * q + k] = Mk;
            if (E_out) E_out[2 * q + k] = Ek;
            if (gain_out) gain_out[2 * q + k] = std::log(Mk) + (double)Ek * ln2;
            if (deg_out) deg_out[2 * q + k] = e0[(size_t)(2 + k) * in + j];
        }
    }
    return PAGAN_OK;
}

void NniRun::fill(pagan_anc_nni_info *info) const {
    std::memset(info, 0, sizeof(*info));
    info->rounds = rounds; info->up_passes = R.info.up_passes; info->chunks = R.info.chunks;
    info->data_type = R.info.data_type; info->states = R.info.states; info->candidates = ncand;
    info->columns = R.info.columns; info->chunk_cols = R.info.chunk_cols; info->device_bytes = R.info.device_bytes;
    info->encode_ms = R.info.encode_ms; info->up_ms = R.info.up_ms; info->down_ms = R.info.down_ms;
    info->nni_ms = nni_ms; info->fold_ms = fold_ms; info->fit_ms = R.info.branch_ms + R.info.fold_ms;
}

int nni_gains(int32_t n, const int32_t *left, const int32_t *right, const double *branch, const char *const *rows, int32_t data_type,
              const float *base_freq, int32_t *kind, double *M, int64_t *E, double *gain, int64_t *degenerate, double *loglik, pagan_anc_nni_info *info_out) {
    const double t0 = wall_s();
    NniRun X;
    int rc = X.setup(n, left, right, branch, rows, data_type, base_freq);
    if (rc != PAGAN_OK) return rc;
    double ll = 0.0;
    if ((rc = X.gains(&ll, M, E, gain, degenerate)) != PAGAN_OK) return rc;
    if (kind) std::copy(X.kind.begin(), X.kind.end(), kind);
    if (loglik) *loglik = ll;
    if (info_out) {
        X.fill(info_out);
        info_out->loglik_start = info_out->loglik_end = ll;
        info_out->fit_ms = 0.0;
        info_out->total_ms = (wall_s() - t0) * 1e3;
    }
    return PAGAN_OK;
}

int nni_search(int32_t n, const int32_t *left, const int32_t *right, const double *branch, const char *const *rows, int32_t data_type,
               const float *base_freq, const pagan_anc_nni_opts *opts, int32_t *left_out, int32_t *right_out, double *branch_out, double *hist_out,
               int32_t hist_cap, pagan_anc_nni_swap *swaps_out, int32_t swap_cap, int32_t *n_swaps, pagan_anc_nni_info *info_out) {
    const double t0 = wall_s();
    pagan_anc_nni_opts o{1e-3, 1e-6, 10.0, 1e-6, 32, 0, 0};
    if (opts) o = *opts;
    const pagan_anc_fit_opts fo{o.t_min, o.t_max, o.tol, o.fit_rounds, 0};
    if (!(o.min_gain >= 0) || o.max_rounds < 0 || !fit_opts_ok(fo) || hist_cap < 0 || swap_cap < 0) return PAGAN_E_ARG;
    NniRun X;
    int rc = X.setup(n, left, right, branch, rows, data_type, base_freq);
    if (rc != PAGAN_OK) return rc;
    const int in = n - 1;
    double ll = 0.0;
    if ((rc = X.up(&ll)) != PAGAN_OK) return rc;
    std::vector<double> hist{ll}, gain((size_t)2 * in), fitted, fit_hist;
    std::vector<int64_t> deg((size_t)2 * in);
    std::vector<int32_t> sel((size_t)in), sel_k((size_t)in), l2((size_t)in), r2((size_t)in);
    std::vector<double> b2((size_t)2 * n - 1);
    std::vector<pagan_anc_nni_swap> swaps;
    int status = PAGAN_ANC_NNI_MAX_ROUNDS;
    for (int round = 0; round < o.max_rounds; ++round) {
        if ((rc = X.gains(&ll, nullptr, nullptr, gain.data(), deg.data())) != PAGAN_OK) return rc;
        const int count = nni_select(n, X.left.data(), X.right.data(), gain.data(), deg.data(), o.min_gain, sel.data(), sel_k.data());
        if (count == 0) { status = PAGAN_ANC_NNI_CONVERGED; break; }
        const std::vector<int32_t> l0 = X.left, r0 = X.right;
        const std::vector<double> b0 = X.branch;
        int applied = count;
        double llc = 0.0;
        for (;;) {                                     // all of them; where that lowers the loglik, the first alone
            std::vector<int32_t> l1 = l0, r1 = r0;
            for (int s = 0; s < applied; ++s) nni_swap_in_place(n, l1, r1, sel[s], sel_k[s]);
            nni_renumber(n, l1, r1, b0.data(), l2.data(), r2.data(), b2.data(), nullptr);
            if ((rc = X.set_tree(l2, r2, b2)) != PAGAN_OK) return rc;
            if ((rc = X.up(&llc)) != PAGAN_OK) return rc;
            if (!(llc < ll) || applied == 1) break;
            applied = 1;
        }
        if (llc < ll || !std::isfinite(llc)) {
            status = PAGAN_ANC_NNI_STALLED;
            if ((rc = X.set_tree(l0, r0, b0)) != PAGAN_OK) return rc;
            break;
        }
        for (int s = 0; s < applied; ++s)
            swaps.push_back({round, sel[s], sel_k[s], applied == count ? 1 : 0, gain[(size_t)2 * (sel[s] - n) + sel_k[s] - 1]});
        ll = llc;
        if (o.fit_rounds > 0) {
            int fit_status = 0;
            const std::vector<double> from = X.branch;
            double fit_ll = 0.0;
            if ((rc = fit_loop(X.R, fo, from.data(), fitted, fit_hist, &fit_ll, &fit_status)) != PAGAN_OK) return rc;
            fitted[(size_t)2 * n - 2] = 0.0;
            // the fit starts from the lengths kept within [t_min, t_max], which may cost more than its rounds regain: then the
            // accepted tree keeps the lengths it has
            const bool keep = fit_ll < ll || !std::isfinite(fit_ll);
            if (!keep) ll = fit_ll;
            if ((rc = X.set_tree(X.left, X.right, keep ? from : fitted)) != PAGAN_OK) return rc;
        }
        hist.push_back(ll);
    }
    std::copy(X.left.begin(), X.left.end(), left_out); std::copy(X.right.begin(), X.right.end(), right_out);
    std::copy(X.branch.begin(), X.branch.end(), branch_out);
    for (size_t k = 0; k < hist.size() && (int64_t)k < hist_cap && hist_out; ++k) hist_out[k] = hist[k];
    for (size_t k = 0; k < swaps.size() && (int64_t)k < swap_cap && swaps_out; ++k) swaps_out[k] = swaps[k];
    if (n_swaps) *n_swaps = (int32_t)swaps.size();
    if (info_out) {
        X.fill(info_out);
        info_out->status = status; info_out->swaps = (int32_t)swaps.size();
        if (o.fit_rounds == 0) info_out->fit_ms = 0.0;                  // (the empty intervals between an up pass's events)
        info_out->loglik_start = hist.front(); info_out->loglik_end = hist.back();
        info_out->total_ms = (wall_s() - t0) * 1e3;
    }
    return (int)hist.size();
}

} // namespace

} // namespace pagan

extern "C" {

int pagan_anc_nni_gains(int32_t n_leaves, const int32_t *left, const int32_t *right, const double *branch, const char *const *rows,
                        int32_t data_type, const float *base_freq, int32_t *kind, double *M, int64_t *E, double *gain, int64_t *degenerate,
                        double *loglik, pagan_anc_nni_info *info) {
    try {
        return pagan::nni_gains(n_leaves, left, right, branch, rows, data_type, base_freq, kind, M, E, gain, degenerate, loglik, info);
    } catch (const std::bad_alloc &) {
        return PAGAN_E_NOMEM;
    }
}

int pagan_anc_nni_search(int32_t n_leaves, const int32_t *left, const int32_t *right, const double *branch, const char *const *rows,
                         int32_t data_type, const float *base_freq, const pagan_anc_nni_opts *opts, int32_t *left_out, int32_t *right_out,
                         double *branch_out, double *loglik_hist, int32_t hist_cap, pagan_anc_nni_swap *swaps, int32_t swap_cap,
                         int32_t *n_swaps, pagan_anc_nni_info *info) {
    try {
        if (!left_out || !right_out || !branch_out) return PAGAN_E_ARG;
        return pagan::nni_search(n_leaves, left, right, branch, rows, data_type, base_freq, opts, left_out, right_out, branch_out, loglik_hist,
                                 hist_cap, swaps, swap_cap, n_swaps, info);
    } catch (const std::bad_alloc &) {
        return PAGAN_E_NOMEM;
    }
}

} // extern "C"
