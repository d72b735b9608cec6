// dp_nj.hip -- the join loop of neighbour joining on the device (include/pagan_host.h, "neighbour joining"; DESIGN.md "Neighbour
// joining").  The symmetric fp64 matrix is resident, row s at M + s * n; the r active clusters sit in the slots 0 .. r-1, with
// their ids and row sums in id[] and R[].
//   nj_row_sums  a wave a row: the header's 64 partial sums and their tree, once.
//   nj_scan      a wave a row s < r - 1: over the slots c > s (every pair once), Q of the pair under the ids' order, the best
//                (Q, lower id, higher id) by the tie rule -- a total order, so neither the lanes' split of the row nor the shape of
//                the reduction (a butterfly of shuffles) changes the result.  One record a row.
//   nj_pick      one workgroup: the best of the r - 1 records (shuffles, then LDS across its four waves); its first thread writes
//                the join record into the log, the pair's slots and d(i, j) for the merge, and the new cluster's id and row sum
//                into the lower slot.
//   nj_merge     a thread a slot k: d(u, k) into the lower slot's row and column, R_k; the cluster of slot r - 1 moves into the
//                upper slot of the pair (its row and column, id, R), so that the active slots stay 0 .. r-2.  A thread reads only
//                its own row and d(i, j) from the pick's record, and no thread writes what another reads.
//   nj_star      one thread: the three clusters left, their lengths, behind the log.
// A join is scan, pick, merge on one stream; the host enqueues all of them, waits once and downloads the log once.  Nothing is
// handed between workgroups inside a launch: no atomics, no flags, nothing depends on timing.  The arithmetic is the header's, in its
// order; the file is compiled without FMA contraction like every other (build.py).
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/pagan_host.h"
#include "dp_hip.h"
#include "host_nj.h"

namespace pagan {

using namespace pgdev;

namespace {

constexpr int kBlock = 256, kWaves = kBlock / 64;

// the tie rule: smaller Q, then the lower first id, then the lower second id
__device__ __forceinline__ bool nj_better(double q, int32_t ia, int32_t ib, double q2, int32_t ia2, int32_t ib2) {
    return q < q2 || (q == q2 && (ia < ia2 || (ia == ia2 && ib < ib2)));
}

// every lane ends with the wave's best record
__device__ __forceinline__ void nj_wave_best(double &q, int32_t &ia, int32_t &ib, int32_t &sa, int32_t &sb) {
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        const double q2 = __shfl_xor(q, s, 64);
        const int32_t ia2 = __shfl_xor(ia, s, 64), ib2 = __shfl_xor(ib, s, 64), sa2 = __shfl_xor(sa, s, 64), sb2 = __shfl_xor(sb, s, 64);
        if (nj_better(q2, ia2, ib2, q, ia, ib)) { q = q2; ia = ia2; ib = ib2; sa = sa2; sb = sb2; }
    }
}

__global__ __launch_bounds__(kBlock) void nj_row_sums(const double *__restrict__ M, uint32_t n, double *__restrict__ R, int32_t *__restrict__ id) {
    const uint32_t lane = threadIdx.x & 63, row = blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (row >= n) return;                                              // (the whole wave)
    const double *m = M + (size_t)row * n;
    double x = 0.0;
    for (uint32_t c = lane; c < n; c += 64) x = x + m[c];              // (the diagonal is stored as 0)
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) x = x + __shfl_down(x, s, 64);   // lanes l < s hold the header's x[l]
    if (lane == 0) { R[row] = x; id[row] = (int32_t)row; }
}

__global__ __launch_bounds__(kBlock) void nj_scan(const double *__restrict__ M, const double *__restrict__ R, const int32_t *__restrict__ id,
                                                  uint32_t n, uint32_t r, NjRowBest *__restrict__ best) {
    const uint32_t lane = threadIdx.x & 63, row = blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (row + 1 >= r) return;                                          // (the whole wave; the last slot has no slot after it)
    const double *m = M + (size_t)row * n;
    const double rm2 = (double)(r - 2), r_row = R[row];
    const int32_t id_row = id[row];
    double bq = INFINITY;
    int32_t ba = INT_MAX, bb = INT_MAX, bs = INT_MAX;
    for (uint32_t c = row + 1 + lane; c < r; c += 64) {
        const double d = m[c], r_c = R[c];
        const int32_t id_c = id[c];
        const bool row_first = id_row < id_c;
        const int32_t ia = row_first ? id_row : id_c, ib = row_first ? id_c : id_row;
        const double q = (rm2 * d - (row_first ? r_row : r_c)) - (row_first ? r_c : r_row);
        if (nj_better(q, ia, ib, bq, ba, bb)) { bq = q; ba = ia; bb = ib; bs = (int32_t)c; }
    }
    int32_t sa = (int32_t)row;
    nj_wave_best(bq, ba, bb, sa, bs);
    if (lane == 0) best[row] = NjRowBest{bq, ba, bb, sa, bs};
}

__global__ __launch_bounds__(kBlock) void nj_pick(const NjRowBest *__restrict__ best, const double *__restrict__ M, double *__restrict__ R,
                                                  int32_t *__restrict__ id, uint32_t n, uint32_t r, uint32_t t, NjPick *__restrict__ cur,
                                                  NjRecord *__restrict__ log) {
    __shared__ NjRowBest part[kWaves];
    double bq = INFINITY;
    int32_t ba = INT_MAX, bb = INT_MAX, sa = INT_MAX, sb = INT_MAX;
    for (uint32_t k = threadIdx.x; k + 1 < r; k += kBlock) {
        const NjRowBest b = best[k];
        if (nj_better(b.q, b.ia, b.ib, bq, ba, bb)) { bq = b.q; ba = b.ia; bb = b.ib; sa = b.sa; sb = b.sb; }
    }
    nj_wave_best(bq, ba, bb, sa, sb);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = NjRowBest{bq, ba, bb, sa, sb};
    __syncthreads();
    if (threadIdx.x != 0) return;
    NjRowBest b = part[0];
    for (int w = 1; w < kWaves; ++w)
        if (nj_better(part[w].q, part[w].ia, part[w].ib, b.q, b.ia, b.ib)) b = part[w];
    if ((uint32_t)b.sa >= r || (uint32_t)b.sb >= r) return;           // (a Q that is no number: nothing is written out of bounds)
    const int32_t si = id[b.sa] == b.ia ? b.sa : b.sb, sj = si == b.sa ? b.sb : b.sa;
    const double dij = M[(size_t)b.sa * n + (uint32_t)b.sb], r_i = R[si], r_j = R[sj];
    const double len_i = dij / 2 + (r_i - r_j) / (2 * (double)(r - 2)), len_j = dij - len_i;
    const double r_u = ((r_i + r_j) - (double)r * dij) / 2;
    const int32_t u = (int32_t)(n + t);
    log[t] = NjRecord{b.ia, b.ib, len_i, len_j};
    *cur = NjPick{dij, si, sj};
    R[b.sa] = r_u;                                                     // (sa < sb: the new cluster takes the lower slot)
    id[b.sa] = u;
}

__global__ __launch_bounds__(kBlock) void nj_merge(double *__restrict__ M, double *__restrict__ R, int32_t *__restrict__ id, uint32_t n,
                                                   uint32_t r, const NjPick *__restrict__ cur) {
    const uint32_t k = blockIdx.x * kBlock + threadIdx.x;
    if (k >= r) return;
    const uint32_t si = (uint32_t)cur->si, sj = (uint32_t)cur->sj;
    if (si >= r || sj >= r || si == sj) return;                         // (the pick wrote nothing)
    const uint32_t keep = min(si, sj), drop = max(si, sj), last = r - 1;
    if (k == keep || k == drop) return;
    const double dij = cur->dij;
    double *mk = M + (size_t)k * n;
    const double dik = mk[si], djk = mk[sj];
    const double duk = ((dik + djk) - dij) / 2;
    const double r_k = ((R[k] - dik) - djk) + duk;
    const uint32_t to = k == last ? drop : k;                           // where cluster k is from here on
    M[(size_t)keep * n + to] = duk;
    M[(size_t)to * n + keep] = duk;
    R[to] = r_k;
    if (k == last) {
        id[drop] = id[last];
    } else if (drop != last) {
        const double v = mk[last];
        M[(size_t)drop * n + k] = v;
        mk[drop] = v;
    }
}

__global__ void nj_star(const double *__restrict__ M, const int32_t *__restrict__ id, uint32_t n, NjStar *__restrict__ star) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    uint32_t s[3] = {0, 1, 2};
    for (int a = 0; a < 2; ++a)                                          // the three slots by id
        for (int b = 0; b < 2 - a; ++b)
            if (id[s[b]] > id[s[b + 1]]) { const uint32_t x = s[b]; s[b] = s[b + 1]; s[b + 1] = x; }
    const double ab = M[(size_t)s[0] * n + s[1]], ac = M[(size_t)s[0] * n + s[2]], bc = M[(size_t)s[1] * n + s[2]];
    NjStar out;
    for (int k = 0; k < 3; ++k) out.ids[k] = id[s[k]];
    out.pad = 0;
    out.len[0] = ((ab + ac) - bc) / 2;
    out.len[1] = ((ab + bc) - ac) / 2;
    out.len[2] = ((ac + bc) - ab) / 2;
    *star = out;
}

struct Device {                     // released on every exit path (the stream has drained before the buffer is freed: dp_hip.h)
    DevBuf mem;
    Stream st;
    std::vector<Event> ev;
};

#define HIPN(x) PG_HIP_CODE(x, "pagan nj", PAGAN_E_INTERNAL)

int run_device(int n, const double *dist, NjRecord *log, NjStar *star, pagan_nj_info *info) {
    const NjLayout L(n);
    const uint32_t joins = (uint32_t)n - 3, N = (uint32_t)n;
    const char *env = std::getenv("PAGAN_NJ_EVENTS");
    const bool stage_events = env && env[0] == '1';                  // (an event between any two launches costs as much as a launch)
    info->device_bytes = (int64_t)L.total;
    std::vector<double> sym((size_t)n * n);
    for (size_t i = 0; i < (size_t)n; ++i) {
        sym[i * n + i] = 0.0;
        for (size_t j = i + 1; j < (size_t)n; ++j) sym[i * n + j] = sym[j * n + i] = dist[i * n + j];
    }
    Device D;
    HIPN(D.st.create(hipStreamNonBlocking));
    D.ev = std::vector<Event>(stage_events ? 3 * (size_t)joins + 1 : 2);
    for (Event &e : D.ev) HIPN(e.create());
    hipStream_t st = D.st;
    HIPN(D.mem.alloc(L.total));
    double *M = (double *)(D.mem.h + L.matrix), *R = (double *)(D.mem.h + L.R);
    int32_t *id = (int32_t *)(D.mem.h + L.id);
    NjRowBest *best = (NjRowBest *)(D.mem.h + L.best);
    NjPick *cur = (NjPick *)(D.mem.h + L.cur);
    NjRecord *d_log = (NjRecord *)(D.mem.h + L.log);
    NjStar *d_star = (NjStar *)(d_log + joins);
    HIPN(hipMemcpyAsync(M, sym.data(), sym.size() * sizeof(double), hipMemcpyHostToDevice, st));
    // all ones: slots and ids of -1, which a merge and the host refuse, wherever a pick finds nothing to write
    HIPN(hipMemsetAsync(cur, 0xFF, sizeof(NjPick), st));
    HIPN(hipMemsetAsync(d_log, 0xFF, (size_t)joins * sizeof(NjRecord) + sizeof(NjStar), st));
    hipLaunchKernelGGL(nj_row_sums, dim3((N + kWaves - 1) / kWaves), dim3(kBlock), 0, st, M, N, R, id);
    size_t e = 0;
    HIPN(hipEventRecord(D.ev[e++], st));
    for (uint32_t t = 0; t < joins; ++t) {
        const uint32_t r = N - t;
        hipLaunchKernelGGL(nj_scan, dim3((r - 1 + kWaves - 1) / kWaves), dim3(kBlock), 0, st, M, R, id, N, r, best);
        if (stage_events) HIPN(hipEventRecord(D.ev[e++], st));
        hipLaunchKernelGGL(nj_pick, dim3(1), dim3(kBlock), 0, st, best, M, R, id, N, r, t, cur, d_log);
        if (stage_events) HIPN(hipEventRecord(D.ev[e++], st));
        hipLaunchKernelGGL(nj_merge, dim3((r + kBlock - 1) / kBlock), dim3(kBlock), 0, st, M, R, id, N, r, cur);
        if (stage_events) HIPN(hipEventRecord(D.ev[e++], st));
        info->scan_entries += (int64_t)r * (r - 1) / 2;
    }
    if (!stage_events) HIPN(hipEventRecord(D.ev[e++], st));
    hipLaunchKernelGGL(nj_star, dim3(1), dim3(64), 0, st, M, id, N, d_star);
    HIPN(hipGetLastError());
    std::vector<char> back((size_t)joins * sizeof(NjRecord) + sizeof(NjStar));
    HIPN(hipMemcpyAsync(back.data(), d_log, back.size(), hipMemcpyDeviceToHost, st));
    HIPN(hipStreamSynchronize(st));
    std::memcpy(log, back.data(), (size_t)joins * sizeof(NjRecord));
    std::memcpy(star, back.data() + (size_t)joins * sizeof(NjRecord), sizeof(NjStar));
    info->launches = (int32_t)(3 * joins + 2);
    float ms = 0;
    HIPN(hipEventElapsedTime(&ms, D.ev[0], D.ev[e - 1]));
    info->loop_ms = ms;
    if (stage_events)
        for (size_t k = 0; k + 1 < e; ++k) {
            HIPN(hipEventElapsedTime(&ms, D.ev[k], D.ev[k + 1]));
            (k % 3 == 0 ? info->scan_ms : k % 3 == 1 ? info->pick_ms : info->merge_ms) += ms;
        }
    return PAGAN_OK;
}

} // namespace

} // namespace pagan

using namespace pagan;

extern "C" {

int pagan_nj_joins(int32_t n, const double *dist, int32_t *join_ids, double *join_len, int32_t star_ids[3], double star_len[3],
                   pagan_nj_info *info_out) {
    if (nj_check_input(n, dist) != PAGAN_OK || !star_ids || !star_len || (n > 3 && (!join_ids || !join_len))) return PAGAN_E_ARG;
    int ndev = 0, device = -1;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return PAGAN_E_NODEVICE;
    if (hipGetDevice(&device) != hipSuccess) return PAGAN_E_NODEVICE;      // the caller's current device; nothing here changes it
    try {
        pagan_nj_info info;
        std::memset(&info, 0, sizeof(info));
        info.n = n; info.joins = n > 3 ? n - 3 : 0;
        if (n == 2) {
            star_ids[0] = 0; star_ids[1] = 1; star_ids[2] = -1;
            star_len[0] = star_len[1] = dist[1] / 2; star_len[2] = 0.0;
        } else {
            std::vector<NjRecord> log((size_t)info.joins);
            NjStar star;
            const int rc = run_device(n, dist, log.data(), &star, &info);
            if (rc != PAGAN_OK) return rc;
            for (int t = 0; t < info.joins; ++t) {
                const NjRecord &j = log[(size_t)t];
                // what the kernels leave for a Q that is no number (distances whose sums overflow) is no join
                if (j.i < 0 || j.i >= j.j || j.j >= n + t) return PAGAN_E_INTERNAL;
                join_ids[2 * t] = j.i; join_ids[2 * t + 1] = j.j;
                join_len[2 * t] = j.len_i; join_len[2 * t + 1] = j.len_j;
            }
            for (int k = 0; k < 3; ++k) { star_ids[k] = star.ids[k]; star_len[k] = star.len[k]; }
        }
        if (info_out) *info_out = info;
        return PAGAN_OK;
    } catch (const std::bad_alloc &) {
        return PAGAN_E_NOMEM;
    }
}

} // extern "C"
