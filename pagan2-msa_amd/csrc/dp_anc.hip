// dp_anc.hip -- ancestral states by marginal likelihood on the device (include/pagan_host.h, "ancestral states by marginal
// likelihood"; DESIGN.md "Ancestral states"): Felsenstein pruning up the tree, the outside pass down, the marginal posterior of
// every internal node in every column.  Columns are independent, so a workgroup owns 64 columns (a lane a column) and walks the
// whole node schedule itself: internal node n + k in the order k = 0 .. n-2 on the way up (children come before parents in the
// walk's ids), the reverse on the way down.  Nothing is handed from one workgroup to another: no flags, no counters, no atomics.
//   pa_encode   the rows arrive as bytes; a thread a (leaf, column) turns a character (codons: three) into a code through the
//               tables of host_anc.cpp and notes whether the leaf holds data there.  Columns past the chunk's end are missing data.
//   pa_up       per node L_v[s] = a[s] b[s] with a, b the children's messages sum_t P[s][t] L[t]; a leaf's message comes from
//               its code (DNA: the sum over its state set; protein, codon: the column P[.][code]), an internal child's from its
//               partial [node][state][column], one coalesced load a state.  The vector is rescaled by the power of two of its
//               largest entry (frexp / ldexp: exact) and the exponent joins the column's running int32.
//   pa_down     per node, from the root: posterior q[s] = L_v[s] O_v[s] over its sum, the first largest state, then for every
//               internal child c with sibling b the outside vector O_c[t] = sum_s (O_v[s] m_b[s]) P_c[s][t], rescaled likewise.
// S = 4 runs in registers, one wave a workgroup.  For S = 20 and 61 the four waves of a workgroup split the states (5 resp. 16
// a wave): what every wave needs of the others -- the largest entry, the terms of the posterior's sum, the vector W -- goes
// through LDS with a __syncthreads, and the partials a wave reads from its neighbours' stores are behind one as well.  The
// entries of P are the same for every lane of a wave: their addresses depend on the node table and the wave's index alone, so
// they are scalar loads (P is kept both ways round, [s][t] and [t][s], so that a wave's states are contiguous in either pass).
// Every sum has a fixed order, nothing depends on timing or on the chunk size.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <map>
#include <new>
#include <vector>

#include "../../include/pagan_host.h"
#include "dp_hip.h"
#include "host_anc.h"
#include "host_guide.h"

namespace pagan {

using namespace pgdev;

namespace {

struct AncArgs {
    unsigned char *has;              // [2n-1][C]
    double *part, *outs;             // [n-1][S][C]
    double *col_lik;                 // [C]
    int32_t *col_exp;                // [C]
    unsigned char *best;             // [n-1][C]
    float *best_p;                   // [n-1][C]
    double *post;                    // [n_post][S][C]
    int32_t n;
    uint32_t C;
};

// What the passes only read: the model and the schedule.  The kernels take these as __restrict__ parameters of their own (they are
// never stored to, so the loads whose addresses are the same in every lane stay scalar loads) and hand them on in this form.
struct AncModel {
    const double *P, *PT, *pi;       // [matrix][s][t], [matrix][t][s], [S]
    const int32_t *nodes;            // [5][n-1]: left, right, matrix of left, matrix of right, slot in `post` or -1
    const unsigned char *codes;      // [n][C]
};

__global__ __launch_bounds__(256) void pa_encode(const unsigned char *__restrict__ raw, const unsigned char *__restrict__ tables, uint32_t n,
                                                 uint32_t C, uint32_t cols, int data_type, unsigned char *__restrict__ codes,
                                                 unsigned char *__restrict__ has) {
    __shared__ unsigned char tab[256 + 64];
    for (uint32_t k = threadIdx.x; k < 256 + 64; k += blockDim.x) tab[k] = tables[k];
    __syncthreads();
    const unsigned char missing = data_type == 1 ? 0 : kAncMissing;
    const uint32_t cpc = data_type == 3 ? 3 : 1;
    const uint64_t items = (uint64_t)n * C;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < items; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t leaf = (uint32_t)(i / C), col = (uint32_t)(i % C);
        unsigned char code = missing;
        if (col < cols) {
            const unsigned char *p = raw + ((uint64_t)leaf * C + col) * cpc;
            if (data_type != 3) code = tab[p[0]];
            else {
                const unsigned a = tab[p[0]], b = tab[p[1]], c = tab[p[2]];
                if (a < 4 && b < 4 && c < 4) code = tab[256 + a * 16 + b * 4 + c];
            }
        }
        codes[i] = code;
        has[i] = code != missing;
    }
}

// a[j] = sum_t P[s0 + j][t] L_child[t] for the wave's states (1 everywhere for a child without data), has = the child's has_data
template <int S, int NS>
__device__ __forceinline__ void pa_message(const AncArgs &A, const AncModel &M, int32_t child, int32_t pm, uint32_t s0, uint64_t col, double (&a)[NS], bool &has) {
    const double *PT = M.PT + (uint64_t)pm * S * S + s0;
    if (child < A.n) {
        const unsigned code = M.codes[(uint64_t)child * A.C + col];
        if constexpr (S == 4) {
            has = code != 0;
#pragma unroll
            for (int j = 0; j < NS; ++j) a[j] = 0.0;
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const double x = (code >> t) & 1u ? 1.0 : 0.0;
#pragma unroll
                for (int j = 0; j < NS; ++j) a[j] += PT[t * S + j] * x;
            }
        } else {
            has = code != kAncMissing;
            const double *col_of = PT + (uint64_t)(has ? code : 0) * S;          // (a lane a code: vector loads)
#pragma unroll
            for (int j = 0; j < NS; ++j) a[j] = s0 + j < (uint32_t)S ? col_of[j] : 0.0;
        }
    } else {
        has = A.has[(uint64_t)child * A.C + col] != 0;
        const double *L = A.part + (uint64_t)(child - A.n) * S * A.C + col;
#pragma unroll
        for (int j = 0; j < NS; ++j) a[j] = 0.0;
#pragma unroll 4
        for (int t = 0; t < S; ++t) {
            const double x = L[(uint64_t)t * A.C];
#pragma unroll
            for (int j = 0; j < NS; ++j) if (s0 + j < (uint32_t)S) a[j] += PT[t * S + j] * x;
        }
    }
    if (!has) {
#pragma unroll
        for (int j = 0; j < NS; ++j) a[j] = 1.0;
    }
}

// the largest of the waves' m, lane by lane (xmax: [W][64]); all waves of the workgroup call it
template <int W>
__device__ __forceinline__ double pa_all_max(double m, double *xmax, uint32_t wave, uint32_t lane) {
    if constexpr (W > 1) {
        xmax[wave * 64 + lane] = m;
        __syncthreads();
        m = xmax[lane];
#pragma unroll
        for (int w = 1; w < W; ++w) m = fmax(m, xmax[w * 64 + lane]);
    }
    return m;
}

// the binary exponent the vector with largest entry m is rescaled by: m 2^-e lies in [1/2, 1); 0 for a vector of zeros
__device__ __forceinline__ int pa_exponent(double m) {
    int e = 0;
    if (m > 0.0) (void)frexp(m, &e);
    return e;
}

template <int S, int W>
__global__ __launch_bounds__(64 * W) void pa_up(AncArgs A, const double *__restrict__ P, const double *__restrict__ PT, const double *__restrict__ pi, const int32_t *__restrict__ nodes,
                                               const unsigned char *__restrict__ codes) {
    const AncModel M{P, PT, pi, nodes, codes};
    constexpr int NS = (S + W - 1) / W;
    __shared__ double xmax[W > 1 ? W * 64 : 1];
    const uint32_t lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), s0 = wave * NS;
    const uint64_t col = (uint64_t)blockIdx.x * 64 + lane;
    const int32_t in = A.n - 1;
    int32_t run = 0;
    for (int32_t k = 0; k < in; ++k) {
        const int32_t l = M.nodes[k], r = M.nodes[in + k], pl = M.nodes[2 * in + k], pr = M.nodes[3 * in + k];
        double a[NS], b[NS];
        bool ha, hb;
        pa_message<S, NS>(A, M, l, pl, s0, col, a, ha);
        pa_message<S, NS>(A, M, r, pr, s0, col, b, hb);
        double m = 0.0;
#pragma unroll
        for (int j = 0; j < NS; ++j) {
            a[j] *= b[j];
            if (s0 + j < (uint32_t)S) m = fmax(m, a[j]);
        }
        m = pa_all_max<W>(m, xmax, wave, lane);
        const int e = ha || hb ? pa_exponent(m) : 0;                // (a node without data keeps its exact ones)
        run += e;
#pragma unroll
        for (int j = 0; j < NS; ++j)
            if (s0 + j < (uint32_t)S) A.part[((uint64_t)k * S + s0 + j) * A.C + col] = ldexp(a[j], -e);
        if (wave == 0) A.has[(uint64_t)(A.n + k) * A.C + col] = ha || hb;
        if constexpr (W > 1) __syncthreads();          // the partial and has_data are the next nodes' input in every wave; xmax is free again
    }
    if (wave == 0) {
        const double *L = A.part + (uint64_t)(in - 1) * S * A.C + col;
        double lik = 0.0;
#pragma unroll 4
        for (int s = 0; s < S; ++s) lik += M.pi[s] * L[(uint64_t)s * A.C];
        A.col_lik[col] = A.has[(uint64_t)(A.n + in - 1) * A.C + col] ? lik : 1.0;      // (a column without data: the exact 1, not pi's sum)
        A.col_exp[col] = run;
    }
}

template <int S, int W>
__global__ __launch_bounds__(64 * W) void pa_down(AncArgs A, const double *__restrict__ P, const double *__restrict__ PT, const double *__restrict__ pi, const int32_t *__restrict__ nodes,
                                               const unsigned char *__restrict__ codes) {
    const AncModel M{P, PT, pi, nodes, codes};
    constexpr int NS = (S + W - 1) / W;
    __shared__ double xmax[W > 1 ? W * 64 : 1];
    __shared__ double xq[W > 1 ? S * 64 : 1];
    const uint32_t lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), s0 = wave * NS;
    const uint64_t col = (uint64_t)blockIdx.x * 64 + lane;
    const int32_t in = A.n - 1;
    for (int32_t k = in - 1; k >= 0; --k) {
        const int32_t l = M.nodes[k], r = M.nodes[in + k], pl = M.nodes[2 * in + k], pr = M.nodes[3 * in + k], slot = M.nodes[4 * in + k];
        double O[NS], q[NS];
#pragma unroll
        for (int j = 0; j < NS; ++j) {
            O[j] = q[j] = 0.0;
            if (s0 + j < (uint32_t)S) {
                const uint64_t at = ((uint64_t)k * S + s0 + j) * A.C + col;
                O[j] = k == in - 1 ? M.pi[s0 + j] : A.outs[at];
                q[j] = A.part[at] * O[j];
            }
        }
        // the posterior's sum and its first largest term, over all states in their order
        double sum = 0.0, top = 0.0;
        int top_s = 0;
        if constexpr (W > 1) {
#pragma unroll
            for (int j = 0; j < NS; ++j) if (s0 + j < (uint32_t)S) xq[(s0 + j) * 64 + lane] = q[j];
            __syncthreads();
            top = xq[lane];
            for (int s = 0; s < S; ++s) {
                const double x = xq[s * 64 + lane];
                sum += x;
                if (x > top) { top = x; top_s = s; }
            }
        } else {
            top = q[0];
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                sum += q[s];
                if (q[s] > top) { top = q[s]; top_s = s; }
            }
        }
        if (wave == 0) {
            A.best[(uint64_t)k * A.C + col] = (unsigned char)top_s;
            A.best_p[(uint64_t)k * A.C + col] = sum > 0.0 ? (float)(top / sum) : 0.0f;
        }
        if (slot >= 0) {
#pragma unroll
            for (int j = 0; j < NS; ++j)
                if (s0 + j < (uint32_t)S) A.post[((uint64_t)slot * S + s0 + j) * A.C + col] = sum > 0.0 ? q[j] / sum : 0.0;
        }
        for (int side = 0; side < 2; ++side) {
            const int32_t c = side ? r : l, b = side ? l : r, pc = side ? pr : pl, pb = side ? pl : pr;
            if (c < A.n) continue;                     // (the same in every thread of the workgroup: the barriers below are uniform)
            double w[NS], o[NS];
            bool hb;
            pa_message<S, NS>(A, M, b, pb, s0, col, w, hb);
#pragma unroll
            for (int j = 0; j < NS; ++j) { w[j] *= O[j]; o[j] = 0.0; }
            const double *Pc = M.P + (uint64_t)pc * S * S + s0;
            if constexpr (W > 1) {
                __syncthreads();                       // every wave has read xq
#pragma unroll
                for (int j = 0; j < NS; ++j) if (s0 + j < (uint32_t)S) xq[(s0 + j) * 64 + lane] = w[j];
                __syncthreads();
#pragma unroll 4
                for (int s = 0; s < S; ++s) {
                    const double x = xq[s * 64 + lane];
#pragma unroll
                    for (int j = 0; j < NS; ++j) if (s0 + j < (uint32_t)S) o[j] += x * Pc[s * S + j];
                }
            } else {
#pragma unroll
                for (int s = 0; s < NS; ++s)
#pragma unroll
                    for (int j = 0; j < NS; ++j) o[j] += w[s] * Pc[s * S + j];
            }
            double m = 0.0;
#pragma unroll
            for (int j = 0; j < NS; ++j) if (s0 + j < (uint32_t)S) m = fmax(m, o[j]);
            m = pa_all_max<W>(m, xmax, wave, lane);
            const int e = pa_exponent(m);
#pragma unroll
            for (int j = 0; j < NS; ++j)
                if (s0 + j < (uint32_t)S) A.outs[((uint64_t)(c - A.n) * S + s0 + j) * A.C + col] = ldexp(o[j], -e);
        }
        if constexpr (W > 1) __syncthreads();          // the outside vectors are the next nodes' input in every wave; xq, xmax are free again
    }
}

struct Device {                     // released on every exit path (the stream has drained before the buffer is freed: dp_hip.h)
    DevBuf mem;
    Stream st;
    Event ev[4];
};

#define HIPA(x) PG_HIP_CODE(x, "pagan anc", PAGAN_E_INTERNAL)

template <int S, int W>
void launch_passes(const AncArgs &A, const AncModel &M, hipStream_t st, hipEvent_t between) {
    hipLaunchKernelGGL((pa_up<S, W>), dim3(A.C / 64), dim3(64 * W), 0, st, A, M.P, M.PT, M.pi, M.nodes, M.codes);
    (void)hipEventRecord(between, st);
    hipLaunchKernelGGL((pa_down<S, W>), dim3(A.C / 64), dim3(64 * W), 0, st, A, M.P, M.PT, M.pi, M.nodes, M.codes);
}

struct Outputs {
    double *col_lik; int32_t *col_exp; double *col_loglik, *loglik; uint8_t *best; float *best_p; uint8_t *has_data; double *post;
};

int reconstruct(int32_t n, const int32_t *left, const int32_t *right, const double *branch, const char *const *rows, int32_t data_type,
                const float *base_freq, uint32_t flags, int32_t n_post, const int32_t *post_nodes, const Outputs &out, pagan_anc_info *info_out) {
    if (flags != 0 || n_post < 0 || (n_post > 0 && !post_nodes)) return PAGAN_E_ARG;
    int64_t chars = 0;
    int type = 0;
    int rc = aln_check_rows(n, rows, data_type, &chars, &type);
    if (rc != PAGAN_OK) return rc;
    rc = anc_check_tree(n, left, right, branch);
    if (rc != PAGAN_OK) return rc;
    const int S = anc_states(type), cpc = type == 3 ? 3 : 1, in = n - 1;
    if (chars % cpc) return PAGAN_E_ARG;
    const int64_t L = chars / cpc;
    std::vector<int32_t> nodes((size_t)5 * in, -1);
    for (int q = 0; q < n_post; ++q) {
        if (post_nodes[q] < n || post_nodes[q] > 2 * n - 2 || nodes[(size_t)4 * in + post_nodes[q] - n] >= 0) return PAGAN_E_ARG;
        nodes[(size_t)4 * in + post_nodes[q] - n] = q;
    }
    // one matrix per distinct branch length
    std::map<double, int> matrix_of;
    for (int v = 0; v < 2 * n - 2; ++v) matrix_of.emplace(branch[v], 0);
    std::vector<double> P(matrix_of.size() * S * S), PT(P.size()), pi(S);
    ModelFactory mf;
    if (anc_factory(type, base_freq, &mf) != PAGAN_OK) return PAGAN_E_INTERNAL;
    std::copy(mf.pi.begin(), mf.pi.begin() + S, pi.begin());
    {
        int at = 0;
        for (auto &e : matrix_of) {
            e.second = at;
            double *p = P.data() + (size_t)at * S * S, *pt = PT.data() + (size_t)at * S * S;
            anc_pmatrix(mf, e.first, p);
            for (int s = 0; s < S; ++s) for (int t = 0; t < S; ++t) pt[t * S + s] = p[s * S + t];
            ++at;
        }
    }
    for (int k = 0; k < in; ++k) {
        nodes[k] = left[k]; nodes[(size_t)in + k] = right[k];
        nodes[(size_t)2 * in + k] = matrix_of[branch[left[k]]]; nodes[(size_t)3 * in + k] = matrix_of[branch[right[k]]];
    }
    const int64_t C = anc_chunk_cols(n, L, S, 0, AncSwitches::read());
    const AncLayout lay(n, S, cpc, C, (int64_t)matrix_of.size(), n_post);
    pagan_anc_info info;
    std::memset(&info, 0, sizeof(info));
    info.data_type = type; info.states = S; info.matrices = (int32_t)matrix_of.size();
    info.columns = L; info.chunk_cols = C; info.chunks = (int32_t)((L + C - 1) / C); info.device_bytes = (int64_t)lay.total;

    int ndev = 0, device = -1;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return PAGAN_E_NODEVICE;
    if (hipGetDevice(&device) != hipSuccess) return PAGAN_E_NODEVICE;      // the caller's current device; nothing here changes it
    unsigned char tables[256 + 64];
    anc_leaf_tables(type, tables, tables + 256);
    Device D;
    HIPA(D.st.create(hipStreamNonBlocking));
    for (Event &e : D.ev) HIPA(e.create());
    hipStream_t st = D.st;
    HIPA(D.mem.alloc(lay.total));
    char *base = D.mem.h;
    AncArgs A;
    AncModel M;
    unsigned char *d_codes = (unsigned char *)(base + lay.codes);
    M.codes = d_codes; A.has = (unsigned char *)(base + lay.has);
    A.part = (double *)(base + lay.part); A.outs = (double *)(base + lay.outs);
    M.P = (double *)(base + lay.P); M.PT = (double *)(base + lay.PT); M.pi = (double *)(base + lay.pi);
    M.nodes = (int32_t *)(base + lay.nodes);
    A.col_lik = (double *)(base + lay.col_lik); A.col_exp = (int32_t *)(base + lay.col_exp);
    A.best = (unsigned char *)(base + lay.best); A.best_p = (float *)(base + lay.best_p); A.post = (double *)(base + lay.post);
    A.n = n; A.C = (uint32_t)C;
    unsigned char *d_raw = (unsigned char *)(base + lay.raw), *d_tables = (unsigned char *)(base + lay.table);
    HIPA(hipMemcpyAsync(d_tables, tables, sizeof(tables), hipMemcpyHostToDevice, st));
    HIPA(hipMemcpyAsync((void *)M.P, P.data(), P.size() * sizeof(double), hipMemcpyHostToDevice, st));
    HIPA(hipMemcpyAsync((void *)M.PT, PT.data(), PT.size() * sizeof(double), hipMemcpyHostToDevice, st));
    HIPA(hipMemcpyAsync((void *)M.pi, pi.data(), pi.size() * sizeof(double), hipMemcpyHostToDevice, st));
    HIPA(hipMemcpyAsync((void *)M.nodes, nodes.data(), nodes.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));

    std::vector<unsigned char> raw((size_t)n * C * cpc);
    std::vector<double> lik((size_t)C), post_chunk(out.post ? (size_t)n_post * S * C : 0);
    std::vector<int32_t> expo((size_t)C);
    const double ln2 = std::log(2.0);
    double total = 0.0;
    for (int64_t c0 = 0; c0 < L; c0 += C) {
        const int64_t cols = std::min(C, L - c0);
        for (int r = 0; r < n; ++r) std::memcpy(raw.data() + (size_t)r * C * cpc, rows[r] + c0 * cpc, (size_t)cols * cpc);
        HIPA(hipMemcpyAsync(d_raw, raw.data(), raw.size(), hipMemcpyHostToDevice, st));
        HIPA(hipEventRecord(D.ev[0], st));
        const uint64_t items = (uint64_t)n * C;
        hipLaunchKernelGGL(pa_encode, dim3((unsigned)std::min<uint64_t>((items + 255) / 256, 1u << 20)), dim3(256), 0, st, d_raw, d_tables,
                           (uint32_t)n, (uint32_t)C, (uint32_t)cols, type, d_codes, A.has);
        HIPA(hipEventRecord(D.ev[1], st));
        if (S == 4) launch_passes<4, 1>(A, M, st, D.ev[2]);
        else if (S == 20) launch_passes<20, 4>(A, M, st, D.ev[2]);
        else launch_passes<61, 4>(A, M, st, D.ev[2]);
        HIPA(hipEventRecord(D.ev[3], st));
        HIPA(hipGetLastError());
        HIPA(hipMemcpyAsync(lik.data(), A.col_lik, (size_t)cols * sizeof(double), hipMemcpyDeviceToHost, st));
        HIPA(hipMemcpyAsync(expo.data(), A.col_exp, (size_t)cols * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        if (out.best) HIPA(hipMemcpy2DAsync(out.best + c0, (size_t)L, A.best, (size_t)C, (size_t)cols, (size_t)in, hipMemcpyDeviceToHost, st));
        if (out.best_p) HIPA(hipMemcpy2DAsync(out.best_p + c0, (size_t)L * sizeof(float), A.best_p, (size_t)C * sizeof(float), (size_t)cols * sizeof(float), (size_t)in, hipMemcpyDeviceToHost, st));
        if (out.has_data) HIPA(hipMemcpy2DAsync(out.has_data + c0, (size_t)L, A.has, (size_t)C, (size_t)cols, (size_t)(2 * n - 1), hipMemcpyDeviceToHost, st));
        if (!post_chunk.empty()) HIPA(hipMemcpyAsync(post_chunk.data(), A.post, post_chunk.size() * sizeof(double), hipMemcpyDeviceToHost, st));
        HIPA(hipStreamSynchronize(st));
        float ms[3] = {0, 0, 0};
        for (int e = 0; e < 3; ++e) HIPA(hipEventElapsedTime(&ms[e], D.ev[e], D.ev[e + 1]));
        info.encode_ms += ms[0]; info.up_ms += ms[1]; info.down_ms += ms[2];
        for (int64_t c = 0; c < cols; ++c) {
            const double ll = std::log(lik[c]) + expo[c] * ln2;
            if (out.col_lik) out.col_lik[c0 + c] = lik[c];
            if (out.col_exp) out.col_exp[c0 + c] = expo[c];
            if (out.col_loglik) out.col_loglik[c0 + c] = ll;
            total += ll;
        }
        for (size_t q = 0; q < (size_t)n_post && out.post; ++q)
            for (int s = 0; s < S; ++s) {
                const double *from = post_chunk.data() + (q * S + s) * C;
                double *to = out.post + (q * L + c0) * S + s;
                for (int64_t c = 0; c < cols; ++c) to[c * S] = from[c];
            }
    }
    if (out.loglik) *out.loglik = total;
    if (info_out) *info_out = info;
    return PAGAN_OK;
}

} // namespace

} // namespace pagan

using namespace pagan;

extern "C" {

int pagan_anc_reconstruct(int32_t n_leaves, const int32_t *left, const int32_t *right, const double *branch, const char *const *rows,
                          int32_t data_type, const float *base_freq, uint32_t flags, int32_t n_post, const int32_t *post_nodes,
                          double *col_lik, int32_t *col_exp, double *col_loglik, double *loglik, uint8_t *best, float *best_p,
                          uint8_t *has_data, double *post, pagan_anc_info *info) {
    try {
        const Outputs out{col_lik, col_exp, col_loglik, loglik, best, best_p, has_data, post};
        return reconstruct(n_leaves, left, right, branch, rows, data_type, base_freq, flags, n_post, post_nodes, out, info);
    } catch (const std::bad_alloc &) {
        return PAGAN_E_NOMEM;
    }
}

} // extern "C"

#include "dp_anc_brlen.inc"
#include "dp_anc_nni.inc"
