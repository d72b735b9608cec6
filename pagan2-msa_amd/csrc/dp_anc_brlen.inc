// dp_anc_brlen.inc -- branch lengths by maximum likelihood (include/pagan_host.h, "branch lengths by maximum likelihood";
// DESIGN.md "Branch lengths by maximum likelihood"), included at the end of dp_anc.hip: pa_encode, pa_up and pa_down above are
// launched as they are.  After the two passes every branch is independent of every other, so nothing here walks the node
// schedule and nothing is handed from one workgroup to another: no flags, no counters, no atomics.
//   pa_out_has      once a chunk and call, a thread a column: out_has[c] = out_has[v] || has_data[b] from the root down, bytes only.
//   pa_branch       a workgroup a (block of 64 columns, branch); a lane a column.  With c the branch's child, v its parent and b
//                   its sibling: W[s] = O_v[s] m_b[s] (pa_message, as pa_down forms it), y_r[s] = sum_t D_r[s][t] L_c[t] for
//                   r = 0, 1, 2 in one sweep over t, f_r = sum_s W[s] y_r[s], then the column's f_1 / f_0 and
//                   f_2 / f_0 - (f_1 / f_0)^2 where it is informative and the exact 0 where not.  S = 4 runs in registers on one
//                   wave; for S = 20 and 61 the four waves split the states as pa_down's do and the terms W[s] y_r[s] go through
//                   LDS behind a __syncthreads to wave 0, which adds them in state order.  The 64 columns are added by the
//                   header's tree (x[i] += x[i + d], d = 32 .. 1: a shuffle a step) and lane 0 stores [block][branch]{g1, g2, count}.
//   pa_branch_fold  a thread a branch adds the blocks in index order onto the running sums, which survive from chunk to chunk.
// D_0 = P, D_1 and D_2 of every distinct length are made on the host and kept [t][s], so that a wave's states are contiguous;
// they are __restrict__ parameters that are never stored to, so their loads stay scalar loads.

namespace pagan {

namespace {

inline double wall_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

__global__ __launch_bounds__(64) void pa_out_has(const unsigned char *__restrict__ has, unsigned char *out, const int32_t *__restrict__ nodes, int32_t n, uint32_t C) {
    const uint64_t col = (uint64_t)blockIdx.x * 64 + threadIdx.x;
    const int32_t in = n - 1;
    out[(uint64_t)(2 * n - 2) * C + col] = 0;
    for (int32_t k = in - 1; k >= 0; --k) {
        const int32_t l = nodes[k], r = nodes[in + k];
        const unsigned char o = out[(uint64_t)(n + k) * C + col];      // (this thread's own store of an earlier step)
        out[(uint64_t)l * C + col] = o | has[(uint64_t)r * C + col];
        out[(uint64_t)r * C + col] = o | has[(uint64_t)l * C + col];
    }
}

struct BranchArgs {
    const unsigned char *out_has;    // [2n-1][C]
    double *block_sums;              // [C / 64][nb][3]
    uint32_t nb;                     // 2n - 2
};

// the header's tree over the wave's 64 columns: x[i] += x[i + d] for i < d, d = 32 .. 1; lane 0 holds the sum
__device__ __forceinline__ double pa_block_sum(double x) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) x = x + __shfl_down(x, d, 64);
    return x;
}

template <int S, int W>
__global__ __launch_bounds__(64 * W) void pa_branch(AncArgs A, BranchArgs B, const double *__restrict__ PT, const double *__restrict__ D1T, const double *__restrict__ D2T,
                                                   const double *__restrict__ pi, const int32_t *__restrict__ branches, const unsigned char *__restrict__ codes) {
    const AncModel M{nullptr, PT, pi, nullptr, codes};
    constexpr int NS = (S + W - 1) / W;
    __shared__ double xq[W > 1 ? S * 64 : 1];
    const uint32_t lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), s0 = wave * NS;
    const uint32_t block = blockIdx.x / B.nb, br = blockIdx.x % B.nb;
    const uint64_t col = (uint64_t)block * 64 + lane;
    // the branch: its child, its parent's index among the internal nodes, its sibling, the matrices of the child and of the sibling
    const int32_t c = branches[br], kv = branches[B.nb + br], b = branches[2 * B.nb + br], mc = branches[3 * B.nb + br], mb = branches[4 * B.nb + br];
    double w[NS], y0[NS], y1[NS], y2[NS];
    bool hb;
    pa_message<S, NS>(A, M, b, mb, s0, col, w, hb);
#pragma unroll
    for (int j = 0; j < NS; ++j) {
        double O = 0.0;
        if (s0 + j < (uint32_t)S) O = kv == A.n - 2 ? pi[s0 + j] : A.outs[((uint64_t)kv * S + s0 + j) * A.C + col];
        w[j] *= O;
        y0[j] = y1[j] = y2[j] = 0.0;
    }
    const uint64_t at = (uint64_t)mc * S * S + s0;
    const double *T0 = PT + at, *T1 = D1T + at, *T2 = D2T + at;
    if (c < A.n) {
        const unsigned code = codes[(uint64_t)c * A.C + col];
        if constexpr (S == 4) {
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const double x = (code >> t) & 1u ? 1.0 : 0.0;
#pragma unroll
                for (int j = 0; j < NS; ++j) {
                    y0[j] += T0[t * S + j] * x;
                    y1[j] += T1[t * S + j] * x;
                    y2[j] += T2[t * S + j] * x;
                }
            }
        } else {
            const uint64_t row = (uint64_t)(code != kAncMissing ? code : 0) * S;      // (a lane a code: vector loads; a leaf without data is no informative column)
#pragma unroll
            for (int j = 0; j < NS; ++j)
                if (s0 + j < (uint32_t)S) { y0[j] = T0[row + j]; y1[j] = T1[row + j]; y2[j] = T2[row + j]; }
        }
    } else {
        const double *L = A.part + (uint64_t)(c - A.n) * S * A.C + col;
#pragma unroll 2
        for (int t = 0; t < S; ++t) {
            const double x = L[(uint64_t)t * A.C];
#pragma unroll
            for (int j = 0; j < NS; ++j)
                if (s0 + j < (uint32_t)S) {
                    y0[j] += T0[t * S + j] * x;
                    y1[j] += T1[t * S + j] * x;
                    y2[j] += T2[t * S + j] * x;
                }
        }
    }
    // f_r = sum_s W[s] y_r[s], s ascending
    double f0 = 0.0, f1 = 0.0, f2 = 0.0;
    if constexpr (W > 1) {
        for (int r = 0; r < 3; ++r) {
#pragma unroll
            for (int j = 0; j < NS; ++j)
                if (s0 + j < (uint32_t)S) xq[(s0 + j) * 64 + lane] = w[j] * (r == 0 ? y0[j] : r == 1 ? y1[j] : y2[j]);
            __syncthreads();
            if (wave == 0) {
                double f = 0.0;
                for (int s = 0; s < S; ++s) f += xq[s * 64 + lane];
                if (r == 0) f0 = f; else if (r == 1) f1 = f; else f2 = f;
            }
            __syncthreads();                           // wave 0 has read xq
        }
        if (wave != 0) return;                         // (after the last barrier)
    } else {
#pragma unroll
        for (int s = 0; s < NS; ++s) { f0 += w[s] * y0[s]; f1 += w[s] * y1[s]; f2 += w[s] * y2[s]; }
    }
    const bool informative = A.has[(uint64_t)c * A.C + col] != 0 && B.out_has[(uint64_t)c * A.C + col] != 0 && f0 > 0.0;
    double x1 = 0.0, x2 = 0.0;
    if (informative) {
        const double q = f1 / f0;
        x1 = q;
        x2 = f2 / f0 - q * q;
    }
    x1 = pa_block_sum(x1);
    x2 = pa_block_sum(x2);
    const int count = __popcll(__ballot(informative));
    if (lane == 0) {
        double *out = B.block_sums + ((uint64_t)block * B.nb + br) * 3;
        out[0] = x1; out[1] = x2; out[2] = (double)count;
    }
}

__global__ __launch_bounds__(64) void pa_branch_fold(const double *__restrict__ block_sums, double *sums, uint32_t nb, uint32_t blocks) {
    const uint32_t br = blockIdx.x * 64 + threadIdx.x;
    if (br >= nb) return;
    for (int r = 0; r < 3; ++r) {
        double s = sums[(uint64_t)br * 3 + r];
        for (uint32_t q = 0; q < blocks; ++q) s += block_sums[((uint64_t)q * nb + br) * 3 + r];
        sums[(uint64_t)br * 3 + r] = s;
    }
}

template <int S, int W>
void launch_stage(int stage, const AncArgs &A, const AncModel &M, const BranchArgs &B, const double *D1T, const double *D2T, const int32_t *branches, hipStream_t st) {
    if (stage == 0) hipLaunchKernelGGL((pa_up<S, W>), dim3(A.C / 64), dim3(64 * W), 0, st, A, M.P, M.PT, M.pi, M.nodes, M.codes);
    else if (stage == 1) hipLaunchKernelGGL((pa_down<S, W>), dim3(A.C / 64), dim3(64 * W), 0, st, A, M.P, M.PT, M.pi, M.nodes, M.codes);
    else hipLaunchKernelGGL((pa_branch<S, W>), dim3(A.C / 64 * B.nb), dim3(64 * W), 0, st, A, B, M.PT, D1T, D2T, M.pi, branches, M.codes);
}

// One call's device state: the rows' codes of every chunk stay resident, the lengths change from pass to pass.
struct BrlenRun {
    enum Mode { UP_ONLY, FULL, DOWN_ONLY };          // DOWN_ONLY: the partials of the last up pass are still there (one chunk, the same lengths)
    int32_t n = 0, in = 0, nb = 0;
    int type = 0, S = 0, cpc = 1;
    int64_t L = 0, C = 0, chunks = 1;
    const int32_t *left = nullptr, *right = nullptr;
    ModelFactory mf;
    Device D;                       // (the buffer before the stream: dp_hip.h)
    Event more[2];
    char *base = nullptr;
    AncFitLayout lay{2, 4, 1, 64, 1, 2};
    pagan_anc_fit_info info;
    std::vector<double> P, PT, D1T, D2T, lik;
    std::vector<int32_t> nodes, branches, expo;
    bool out_has_done = false;
    int extra_matrices = 0;         // (set before setup) room behind the matrices of the distinct lengths that set_lengths leaves alone

    void set_tree(const int32_t *left_, const int32_t *right_);
    int setup(int32_t n_, const int32_t *left_, const int32_t *right_, const double *branch, const char *const *rows, int32_t data_type, const float *base_freq);
    int set_lengths(const double *branch);
    int pass(Mode mode, double *loglik);
    int read_sums(double *g1, double *g2, int64_t *informative);
};

int BrlenRun::setup(int32_t n_, const int32_t *left_, const int32_t *right_, const double *branch, const char *const *rows, int32_t data_type, const float *base_freq) {
    int64_t chars = 0;
    int rc = aln_check_rows(n_, rows, data_type, &chars, &type);
    if (rc != PAGAN_OK) return rc;
    rc = anc_check_tree(n_, left_, right_, branch);
    if (rc != PAGAN_OK) return rc;
    n = n_; in = n - 1; nb = 2 * n - 2;
    S = anc_states(type); cpc = type == 3 ? 3 : 1;
    if (chars % cpc) return PAGAN_E_ARG;
    L = chars / cpc;
    if (anc_factory(type, base_freq, &mf) != PAGAN_OK) return PAGAN_E_INTERNAL;
    C = anc_chunk_cols(n, L, S, 0, AncSwitches::read());
    chunks = std::max<int64_t>(1, (L + C - 1) / C);
    if ((uint64_t)(C / 64) * (uint64_t)nb > 0x7fffffffull) return PAGAN_E_ARG;       // pa_branch's grid
    lay = AncFitLayout(n, S, cpc, C, chunks, nb + extra_matrices);
    std::memset(&info, 0, sizeof(info));
    info.data_type = type; info.states = S; info.columns = L; info.chunk_cols = C; info.chunks = (int32_t)chunks; info.device_bytes = (int64_t)lay.total;
    set_tree(left_, right_);
    lik.resize((size_t)C); expo.resize((size_t)C);

    int ndev = 0, device = -1;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return PAGAN_E_NODEVICE;
    if (hipGetDevice(&device) != hipSuccess) return PAGAN_E_NODEVICE;
    unsigned char tables[256 + 64];
    anc_leaf_tables(type, tables, tables + 256);
    HIPA(D.st.create(hipStreamNonBlocking));
    for (Event &e : D.ev) HIPA(e.create());
    for (Event &e : more) HIPA(e.create());
    hipStream_t st = D.st;
    HIPA(D.mem.alloc(lay.total));
    base = D.mem.h;
    HIPA(hipMemcpyAsync(base + lay.table, tables, sizeof(tables), hipMemcpyHostToDevice, st));
    HIPA(hipMemcpyAsync(base + lay.pi, mf.pi.data(), (size_t)S * sizeof(double), hipMemcpyHostToDevice, st));
    std::vector<unsigned char> raw((size_t)n * C * cpc);
    for (int64_t ch = 0; ch < chunks; ++ch) {
        const int64_t c0 = ch * C, cols = std::max<int64_t>(0, std::min(C, L - c0));
        for (int r = 0; r < n; ++r) std::memcpy(raw.data() + (size_t)r * C * cpc, rows[r] + c0 * cpc, (size_t)cols * cpc);
        HIPA(hipMemcpyAsync(base + lay.raw, raw.data(), raw.size(), hipMemcpyHostToDevice, st));
        HIPA(hipEventRecord(D.ev[0], st));
        const uint64_t items = (uint64_t)n * C;
        hipLaunchKernelGGL(pa_encode, dim3((unsigned)std::min<uint64_t>((items + 255) / 256, 1u << 20)), dim3(256), 0, st, (const unsigned char *)(base + lay.raw),
                           (const unsigned char *)(base + lay.table), (uint32_t)n, (uint32_t)C, (uint32_t)cols, type,
                           (unsigned char *)(base + lay.codes) + (size_t)ch * n * C, (unsigned char *)(base + lay.has) + (size_t)ch * (2 * n - 1) * C);
        HIPA(hipEventRecord(D.ev[1], st));
        HIPA(hipGetLastError());
        HIPA(hipStreamSynchronize(st));                // `raw` is filled again
        float ms = 0;
        HIPA(hipEventElapsedTime(&ms, D.ev[0], D.ev[1]));
        info.encode_ms += ms;
    }
    return PAGAN_OK;
}

// the topology's half of the node and branch tables (set_lengths fills in the matrices); out_has follows the tree
void BrlenRun::set_tree(const int32_t *left_, const int32_t *right_) {
    left = left_; right = right_;
    nodes.assign((size_t)5 * in, -1);
    branches.assign((size_t)5 * nb, 0);
    for (int k = 0; k < in; ++k) {
        nodes[k] = left[k]; nodes[(size_t)in + k] = right[k];
        for (int side = 0; side < 2; ++side) {
            const int32_t c = side ? right[k] : left[k], b = side ? left[k] : right[k];
            branches[c] = c; branches[(size_t)nb + c] = k; branches[(size_t)2 * nb + c] = b;      // (branch c: the one above node c)
        }
    }
    out_has_done = false;
}

// the matrices of these lengths, one set per distinct length, and the tables that name them; the stream is idle on entry and on return
int BrlenRun::set_lengths(const double *branch) {
    std::map<double, int> matrix_of;
    for (int v = 0; v < nb; ++v) matrix_of.emplace(branch[v], 0);
    const size_t SS = (size_t)S * S;
    P.resize(matrix_of.size() * SS); PT.resize(P.size()); D1T.resize(P.size()); D2T.resize(P.size());
    std::vector<double> d(SS);
    int at = 0;
    for (auto &e : matrix_of) {
        e.second = at;
        double *p = P.data() + at * SS;
        anc_pmatrix(mf, e.first, p);
        for (int s = 0; s < S; ++s) for (int t = 0; t < S; ++t) PT[at * SS + (size_t)t * S + s] = p[(size_t)s * S + t];
        for (int order = 1; order <= 2; ++order) {
            anc_pmatrix_deriv(mf, e.first, order, d.data());
            double *to = (order == 1 ? D1T : D2T).data() + at * SS;
            for (int s = 0; s < S; ++s) for (int t = 0; t < S; ++t) to[(size_t)t * S + s] = d[(size_t)s * S + t];
        }
        ++at;
    }
    for (int k = 0; k < in; ++k) {
        nodes[(size_t)2 * in + k] = matrix_of[branch[left[k]]]; nodes[(size_t)3 * in + k] = matrix_of[branch[right[k]]];
    }
    for (int c = 0; c < nb; ++c) {
        branches[(size_t)3 * nb + c] = matrix_of[branch[c]]; branches[(size_t)4 * nb + c] = matrix_of[branch[branches[(size_t)2 * nb + c]]];
    }
    hipStream_t st = D.st;
    const size_t bytes = P.size() * sizeof(double);
    HIPA(hipMemcpyAsync(base + lay.P, P.data(), bytes, hipMemcpyHostToDevice, st));
    HIPA(hipMemcpyAsync(base + lay.PT, PT.data(), bytes, hipMemcpyHostToDevice, st));
    HIPA(hipMemcpyAsync(base + lay.D1T, D1T.data(), bytes, hipMemcpyHostToDevice, st));
    HIPA(hipMemcpyAsync(base + lay.D2T, D2T.data(), bytes, hipMemcpyHostToDevice, st));
    HIPA(hipMemcpyAsync(base + lay.nodes, nodes.data(), nodes.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
    HIPA(hipMemcpyAsync(base + lay.branches, branches.data(), branches.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
    HIPA(hipStreamSynchronize(st));
    return PAGAN_OK;
}

int BrlenRun::pass(Mode mode, double *loglik) {
    hipStream_t st = D.st;
    AncArgs A;
    AncModel M;
    BranchArgs B;
    A.part = (double *)(base + lay.part); A.outs = (double *)(base + lay.outs);
    A.col_lik = (double *)(base + lay.col_lik); A.col_exp = (int32_t *)(base + lay.col_exp);
    A.best = (unsigned char *)(base + lay.best); A.best_p = (float *)(base + lay.best_p); A.post = nullptr;
    A.n = n; A.C = (uint32_t)C;
    M.P = (double *)(base + lay.P); M.PT = (double *)(base + lay.PT); M.pi = (double *)(base + lay.pi); M.nodes = (int32_t *)(base + lay.nodes);
    const double *d1t = (double *)(base + lay.D1T), *d2t = (double *)(base + lay.D2T);
    const int32_t *d_branches = (int32_t *)(base + lay.branches);
    double *sums = (double *)(base + lay.sums);
    B.block_sums = (double *)(base + lay.block_sums); B.nb = (uint32_t)nb;
    auto stage = [&](int which) {
        if (S == 4) launch_stage<4, 1>(which, A, M, B, d1t, d2t, d_branches, st);
        else if (S == 20) launch_stage<20, 4>(which, A, M, B, d1t, d2t, d_branches, st);
        else launch_stage<61, 4>(which, A, M, B, d1t, d2t, d_branches, st);
    };
    if (mode != UP_ONLY) HIPA(hipMemsetAsync(sums, 0, (size_t)nb * 3 * sizeof(double), st));
    const double ln2 = std::log(2.0);
    double total = 0.0;
    hipEvent_t ev[5] = {D.ev[0], D.ev[1], D.ev[2], D.ev[3], more[0]};
    for (int64_t ch = 0; ch < chunks; ++ch) {
        const int64_t c0 = ch * C, cols = std::max<int64_t>(0, std::min(C, L - c0));
        A.has = (unsigned char *)(base + lay.has) + (size_t)ch * (2 * n - 1) * C;
        M.codes = (unsigned char *)(base + lay.codes) + (size_t)ch * n * C;
        unsigned char *out_has = (unsigned char *)(base + lay.out_has) + (size_t)ch * (2 * n - 1) * C;
        B.out_has = out_has;
        HIPA(hipEventRecord(ev[0], st));
        if (mode != DOWN_ONLY) stage(0);
        HIPA(hipEventRecord(ev[1], st));
        if (mode != UP_ONLY) {
            if (!out_has_done) hipLaunchKernelGGL(pa_out_has, dim3(A.C / 64), dim3(64), 0, st, A.has, out_has, M.nodes, A.n, A.C);
            stage(1);
        }
        HIPA(hipEventRecord(ev[2], st));
        if (mode != UP_ONLY) stage(2);
        HIPA(hipEventRecord(ev[3], st));
        if (mode != UP_ONLY) hipLaunchKernelGGL(pa_branch_fold, dim3((nb + 63) / 64), dim3(64), 0, st, B.block_sums, sums, (uint32_t)nb, (uint32_t)(C / 64));
        HIPA(hipEventRecord(ev[4], st));
        HIPA(hipGetLastError());
        if (mode != DOWN_ONLY) {
            HIPA(hipMemcpyAsync(lik.data(), A.col_lik, (size_t)cols * sizeof(double), hipMemcpyDeviceToHost, st));
            HIPA(hipMemcpyAsync(expo.data(), A.col_exp, (size_t)cols * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        }
        HIPA(hipStreamSynchronize(st));
        float ms[4] = {0, 0, 0, 0};
        for (int e = 0; e < 4; ++e) HIPA(hipEventElapsedTime(&ms[e], ev[e], ev[e + 1]));
        info.up_ms += ms[0]; info.down_ms += ms[1]; info.branch_ms += ms[2]; info.fold_ms += ms[3];
        if (mode != DOWN_ONLY)
            for (int64_t c = 0; c < cols; ++c) total += std::log(lik[c]) + expo[c] * ln2;       // (pagan_anc_reconstruct's sum)
    }
    if (mode != UP_ONLY) out_has_done = true;
    if (mode != DOWN_ONLY) { ++info.up_passes; if (loglik) *loglik = total; }
    if (mode != UP_ONLY) ++info.rounds;
    return PAGAN_OK;
}

// g1, g2, informative [2n-1] by node id (the root's entries 0) from the running sums of the last pass
int BrlenRun::read_sums(double *g1, double *g2, int64_t *informative) {
    std::vector<double> sums((size_t)nb * 3);
    HIPA(hipMemcpy(sums.data(), base + lay.sums, sums.size() * sizeof(double), hipMemcpyDeviceToHost));
    for (int c = 0; c <= nb; ++c) {
        if (g1) g1[c] = c < nb ? sums[(size_t)c * 3] : 0.0;
        if (g2) g2[c] = c < nb ? sums[(size_t)c * 3 + 1] : 0.0;
        if (informative) informative[c] = c < nb ? (int64_t)sums[(size_t)c * 3 + 2] : 0;
    }
    return PAGAN_OK;
}

int branch_derivs(int32_t n, const int32_t *left, const int32_t *right, const double *branch, const char *const *rows, int32_t data_type,
                  const float *base_freq, double *g1, double *g2, int64_t *informative, double *loglik, pagan_anc_fit_info *info_out) {
    const double t0 = wall_s();
    BrlenRun R;
    int rc = R.setup(n, left, right, branch, rows, data_type, base_freq);
    if (rc != PAGAN_OK) return rc;
    if ((rc = R.set_lengths(branch)) != PAGAN_OK) return rc;
    double ll = 0.0;
    if ((rc = R.pass(BrlenRun::FULL, &ll)) != PAGAN_OK) return rc;
    if ((rc = R.read_sums(g1, g2, informative)) != PAGAN_OK) return rc;
    if (loglik) *loglik = ll;
    R.info.loglik_start = R.info.loglik_end = ll;
    R.info.total_ms = (wall_s() - t0) * 1e3;
    if (info_out) *info_out = R.info;
    return PAGAN_OK;
}

// The fit's loop on a run that is set up: from branch_in, at most o.max_rounds rounds.  t [2n-1] the lengths it ends at, hist the
// accepted logliks (the start first), ll the last of them.
int fit_loop(BrlenRun &R, const pagan_anc_fit_opts &o, const double *branch_in, std::vector<double> &t, std::vector<double> &hist, double *ll_out, int *status_out) {
    int rc;
    const int n = R.n, nb = R.nb, rl = R.left[n - 2], rr = R.right[n - 2];
    auto bounded = [&](double x) { return std::min(std::max(x, o.t_min), o.t_max); };
    // the parameters: every branch but the root's two, and tau in their place; p is the root's proportion of branch_in
    std::vector<double> step((size_t)nb + 1), cand((size_t)nb + 1), g1((size_t)nb + 1), g2((size_t)nb + 1);
    t.assign(branch_in, branch_in + nb + 1);
    t[nb] = 0.0;
    const double tau_in = branch_in[rl] + branch_in[rr], p = tau_in > 0 ? branch_in[rl] / tau_in : 0.5;
    auto split = [&](double tau, std::vector<double> &to) { to[rl] = tau * p; to[rr] = tau - to[rl]; };
    for (int c = 0; c < nb; ++c) if (c != rl && c != rr) t[c] = bounded(t[c]);
    if (bounded(tau_in) != tau_in) split(bounded(tau_in), t);
    hist.clear();
    double ll = 0.0;
    if ((rc = R.set_lengths(t.data())) != PAGAN_OK) return rc;
    if ((rc = R.pass(BrlenRun::UP_ONLY, &ll)) != PAGAN_OK) return rc;
    hist.push_back(ll);
    int status = PAGAN_ANC_FIT_MAX_ROUNDS;
    for (int round = 0; round < o.max_rounds; ++round) {
        if ((rc = R.pass(R.chunks == 1 ? BrlenRun::DOWN_ONLY : BrlenRun::FULL, nullptr)) != PAGAN_OK) return rc;
        if ((rc = R.read_sums(g1.data(), g2.data(), nullptr)) != PAGAN_OK) return rc;
        const double tau = t[rl] + t[rr], tau_step = pagan_anc_branch_step(tau, g1[rl], g2[rl], o.t_min, o.t_max);
        double moved = std::fabs(tau_step - tau) / std::max(tau, o.t_min);
        for (int c = 0; c < nb; ++c) {
            if (c == rl || c == rr) continue;
            step[c] = pagan_anc_branch_step(t[c], g1[c], g2[c], o.t_min, o.t_max);
            moved = std::max(moved, std::fabs(step[c] - t[c]) / std::max(t[c], o.t_min));
        }
        if (moved <= o.tol) { status = PAGAN_ANC_FIT_CONVERGED; break; }
        bool accepted = false;
        double alpha = 1.0, llc = 0.0;
        for (int halvings = 0; halvings <= 5 && !accepted; ++halvings, alpha *= 0.5) {
            for (int c = 0; c < nb; ++c)
                if (c != rl && c != rr) cand[c] = alpha == 1.0 ? step[c] : bounded(t[c] + alpha * (step[c] - t[c]));
            split(alpha == 1.0 ? tau_step : bounded(tau + alpha * (tau_step - tau)), cand);
            cand[nb] = 0.0;
            if ((rc = R.set_lengths(cand.data())) != PAGAN_OK) return rc;
            if ((rc = R.pass(BrlenRun::UP_ONLY, &llc)) != PAGAN_OK) return rc;
            accepted = !(llc < ll);
        }
        if (!accepted || !std::isfinite(llc)) { status = PAGAN_ANC_FIT_STALLED; break; }
        t = cand; ll = llc;
        hist.push_back(ll);
    }
    *ll_out = ll; *status_out = status;
    return PAGAN_OK;
}

inline bool fit_opts_ok(const pagan_anc_fit_opts &o) {
    return o.t_min > 0 && o.t_max >= o.t_min && std::isfinite(o.t_max) && o.tol >= 0 && o.max_rounds >= 0;
}

int fit_branches(int32_t n, const int32_t *left, const int32_t *right, const double *branch_in, const char *const *rows, int32_t data_type,
                 const float *base_freq, const pagan_anc_fit_opts *opts, double *branch_out, double *hist_out, int32_t hist_cap, pagan_anc_fit_info *info_out) {
    const double t0 = wall_s();
    pagan_anc_fit_opts o{1e-6, 10.0, 1e-6, 32, 0};
    if (opts) o = *opts;
    if (!fit_opts_ok(o) || hist_cap < 0) return PAGAN_E_ARG;
    BrlenRun R;
    int rc = R.setup(n, left, right, branch_in, rows, data_type, base_freq);
    if (rc != PAGAN_OK) return rc;
    std::vector<double> t, hist;
    double ll = 0.0;
    int status = 0;
    if ((rc = fit_loop(R, o, branch_in, t, hist, &ll, &status)) != PAGAN_OK) return rc;
    if (branch_out) std::copy(t.begin(), t.end(), branch_out);
    for (size_t k = 0; k < hist.size() && (int64_t)k < hist_cap && hist_out; ++k) hist_out[k] = hist[k];
    R.info.status = status; R.info.loglik_start = hist.front(); R.info.loglik_end = ll;
    R.info.total_ms = (wall_s() - t0) * 1e3;
    if (info_out) *info_out = R.info;
    return (int)hist.size();
}

} // namespace

} // namespace pagan

extern "C" {

int pagan_anc_branch_derivs(int32_t n_leaves, const int32_t *left, const int32_t *right, const double *branch, const char *const *rows,
                            int32_t data_type, const float *base_freq, double *g1, double *g2, int64_t *informative, double *loglik,
                            pagan_anc_fit_info *info) {
    try {
        return pagan::branch_derivs(n_leaves, left, right, branch, rows, data_type, base_freq, g1, g2, informative, loglik, info);
    } catch (const std::bad_alloc &) {
        return PAGAN_E_NOMEM;
    }
}

int pagan_anc_fit_branches(int32_t n_leaves, const int32_t *left, const int32_t *right, const double *branch_in, const char *const *rows,
                           int32_t data_type, const float *base_freq, const pagan_anc_fit_opts *opts, double *branch_out,
                           double *loglik_hist, int32_t hist_cap, pagan_anc_fit_info *info) {
    try {
        return pagan::fit_branches(n_leaves, left, right, branch_in, rows, data_type, base_freq, opts, branch_out, loglik_hist, hist_cap, info);
    } catch (const std::bad_alloc &) {
        return PAGAN_E_NOMEM;
    }
}

} // extern "C"
