// dp_guide.hip -- pairwise k-mer distances on the device, the input of the guide tree (include/pagan_host.h, "guide tree";
// DESIGN.md "Guide tree").  All pairs of N sequences are N (N - 1) / 2 independent intersections of sorted lists:
//   pgd_pack      one thread per position of the concatenated cleaned letters: the u64 code of the window that starts there, or
//                 all ones where the window holds a letter that is no core letter or crosses the sequence's end;
//   rocPRIM       segmented radix sort of the keys, a segment per sequence, over the code's bits and one more (the bit that
//                 only the all-ones key has set, so that those sort behind every code);
//   pgd_kmers     per sequence, the number of keys that are codes (a binary search for the first all-ones key);
//   pgd_heads / rocPRIM exclusive scan / pgd_emit / pgd_counts
//                 run-length compression into one (code u64, count u32) list per sequence: a run starts where the key differs
//                 from its predecessor OR the segment starts, so no run crosses a sequence boundary;
//   pgd_pairs     one workgroup per pair x < y; its waves take the shorter list in chunks of 64 entries (wave w the chunks
//                 w, w + W, ...), find the chunk's code range in the longer list with two wave-uniform galloping searches that
//                 start where the wave's previous chunk began, and every lane then searches its own code inside that window.
//                 min(count, count) is summed per lane, across the wave by shuffles, across the waves through LDS, and stored
//                 once by one lane: integers, no atomics, nothing depends on timing.  At most 2^20 workgroups a launch: beyond
//                 that many pairs a workgroup goes on to the pair 2^20 further on.
// Everything indexes positions and entries with 32 bits (the header's limits are checked before anything is allocated); the
// pair index of a workgroup is turned into (x, y) by a binary search over exact 64-bit integers.
#include <hip/hip_runtime.h>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/device/device_segmented_radix_sort.hpp>

#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "../../include/pagan_host.h"
#include "dp_hip.h"
#include "host_guide.h"

namespace pagan {

using namespace pgdev;

namespace {

constexpr uint64_t kNoKmer = ~0ull;
constexpr int kChunk = PAGAN_GUIDE_PAIR_CHUNK;
// workgroups of one pgd_pairs launch: with the 1,024 threads a workgroup has at most, 2^30 threads, inside what a launch takes
// (grid x block < 2^32); far more workgroups than the chip holds at a time, so the cap costs nothing
constexpr uint64_t kMaxPairGroups = 1u << 20;
static_assert(kChunk == 64, "a chunk is one entry per lane of a wave");

__global__ void pgd_pack(const unsigned char *letters, uint32_t total, const uint32_t *off, int n, int k, int bits,
                         uint64_t *keys, uint32_t *seg) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= total) return;
    int lo = 0, hi = n;                                   // the sequence of p: off[lo] <= p < off[hi] (empty sequences have no p)
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (off[mid] <= p) lo = mid; else hi = mid;
    }
    uint64_t key = kNoKmer;
    if ((uint64_t)p + (uint64_t)k <= (uint64_t)off[lo + 1]) {
        uint64_t code = 0;
        bool ok = true;
        for (int j = 0; j < k; ++j) {
            const unsigned c = letters[p + j];
            ok = ok && c != kGuideNoLetter;
            code = (code << bits) | (uint64_t)(c & 31u);
        }
        if (ok) key = code;
    }
    keys[p] = key;
    seg[p] = (uint32_t)lo;
}

__global__ void pgd_kmers(const uint64_t *keys, const uint32_t *off, int n, uint32_t *kmers) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n) return;
    uint32_t lo = off[s], hi = off[s + 1];
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (keys[mid] != kNoKmer) lo = mid + 1; else hi = mid;
    }
    kmers[s] = lo - off[s];
}

// head[p] = 1 where a run starts; head[total] = 0 so that the scan also gives the number of runs
__global__ void pgd_heads(const uint64_t *keys, const uint32_t *seg, const uint32_t *off, uint32_t total, uint32_t *head) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p > total) return;
    uint32_t h = 0;
    if (p < total) {
        const uint64_t key = keys[p];
        h = key != kNoKmer && (p == off[seg[p]] || keys[p - 1] != key);
    }
    head[p] = h;
}

__global__ void pgd_emit(const uint64_t *keys, const uint32_t *head, const uint32_t *pos, const uint32_t *off, uint32_t total, int n,
                         uint64_t *codes, uint32_t *run_start, uint32_t *list_off) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p < total && head[p]) {
        const uint32_t r = pos[p];
        codes[r] = keys[p];
        run_start[r] = p;
    }
    if (p <= (uint32_t)n) list_off[p] = pos[off[p]];      // (off[p] <= total, and pos has total + 1 entries)
}

__global__ void pgd_counts(const uint32_t *run_start, const uint32_t *seg, const uint32_t *off, const uint32_t *kmers,
                           const uint32_t *list_off, const uint32_t *n_runs, uint32_t total, uint32_t *counts) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;       // (a thread a position: the number of runs stays on the device)
    if (r >= total || r >= *n_runs) return;
    const uint32_t p = run_start[r], s = seg[p];
    const uint32_t next = r + 1 < list_off[s + 1] ? run_start[r + 1] : off[s] + kmers[s];
    counts[r] = next - p;
}

__device__ __forceinline__ uint64_t uniform64(uint64_t v) {
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v), hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
    return ((uint64_t)hi << 32) | lo;
}

// first index in [from, n] whose code is >= key (kUpper: > key); every code before `from` is below that bound.  Doubling steps
// from `from`, then a binary search inside the last step.
template <bool kUpper>
__device__ __forceinline__ uint32_t gallop(const uint64_t *B, uint32_t from, uint32_t n, uint64_t key) {
    uint32_t lo = from, hi;
    uint64_t step = kChunk;
    for (;;) {
        const uint64_t probe = (uint64_t)lo + step - 1;
        if (probe >= n) { hi = n; break; }
        const uint64_t v = B[probe];
        if (kUpper ? v > key : v >= key) { hi = (uint32_t)probe; break; }
        lo = (uint32_t)probe + 1;
        step <<= 1;
    }
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        const uint64_t v = B[mid];
        if (kUpper ? v <= key : v < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(1024) void pgd_pairs(const uint64_t *codes, const uint32_t *counts, const uint32_t *list_off, int n,
                                                  uint64_t n_pairs, uint32_t *shared_out) {
    __shared__ uint32_t part[16];
    const uint64_t N = (uint64_t)n;
    // (the grid is capped at kMaxPairGroups: a workgroup takes the pairs blockIdx.x, blockIdx.x + gridDim.x, ...)
    for (uint64_t pair = blockIdx.x; pair < n_pairs; pair += gridDim.x) {
        // pair index -> (x, y), x < y: row x starts at x (2 n - x - 1) / 2; the largest x whose start is <= the index
        uint32_t xl = 0, xh = (uint32_t)n - 2;
        while (xl < xh) {
            const uint64_t mid = ((uint64_t)xl + xh + 1) >> 1;
            if (mid * (2 * N - mid - 1) / 2 <= pair) xl = (uint32_t)mid; else xh = (uint32_t)mid - 1;
        }
        const uint32_t x = xl, y = x + 1 + (uint32_t)(pair - (uint64_t)x * (2 * N - x - 1) / 2);
        uint32_t a0 = list_off[x], nA = list_off[x + 1] - a0, b0 = list_off[y], nB = list_off[y + 1] - b0;
        if (nA > nB) { uint32_t t = a0; a0 = b0; b0 = t; t = nA; nA = nB; nB = t; }
        const uint64_t *A = codes + a0, *B = codes + b0;
        const uint32_t *cA = counts + a0, *cB = counts + b0;
        const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
        uint32_t sum = 0, from = 0;
        for (uint32_t c = wave * kChunk; c < nA; c += waves * kChunk) {
            const uint32_t i = c + lane, last = min(c + kChunk - 1, nA - 1);
            const bool have = i < nA;
            const uint64_t code = A[have ? i : last];
            const uint64_t first_code = uniform64(code), last_code = uniform64(__shfl(code, (int)(last - c)));
            const uint32_t wlo = gallop<false>(B, from, nB, first_code);
            const uint32_t whi = gallop<true>(B, wlo, nB, last_code);
            from = wlo;
            uint32_t lo = wlo, hi = whi;
            while (lo < hi) {
                const uint32_t mid = lo + ((hi - lo) >> 1);
                if (B[mid] < code) lo = mid + 1; else hi = mid;
            }
            if (have && lo < whi && B[lo] == code) sum += min(cA[i], cB[lo]);
        }
        for (int o = 32; o > 0; o >>= 1) sum += __shfl_down(sum, o);
        if (lane == 0) part[wave] = sum;
        __syncthreads();
        if (threadIdx.x == 0) {
            uint32_t s = 0;
            for (uint32_t w = 0; w < waves; ++w) s += part[w];
            shared_out[pair] = s;
        }
        __syncthreads();                                      // (part is written again for the workgroup's next pair)
    }
}

// the device buffers of one call, carved from one allocation (offsets: an array of no bytes takes none)
struct Layout {
    size_t letters, off, kmers, list_off, keys_in, keys_out, seg, head, pos, run_start, counts, pairs, tmp, total;
    Layout(int64_t n, int64_t T, size_t tmp_bytes) {
        Carve c{nullptr};
        letters = c.skip((size_t)T);
        off = c.skip(4 * (size_t)(n + 1)); kmers = c.skip(4 * (size_t)n); list_off = c.skip(4 * (size_t)(n + 1));
        keys_in = c.skip(8 * (size_t)T);               // after the sort: the lists' codes
        keys_out = c.skip(8 * (size_t)T);
        seg = c.skip(4 * (size_t)T); head = c.skip(4 * (size_t)(T + 1)); pos = c.skip(4 * (size_t)(T + 1));
        run_start = c.skip(4 * (size_t)T); counts = c.skip(4 * (size_t)T);
        pairs = c.skip(4 * (size_t)(n * (n - 1) / 2));
        tmp = c.skip(tmp_bytes);
        total = c.cur;
    }
};

// an estimate of what the library calls ask for (the sort's second key buffer and three index arrays over the segments, the
// scan's block prefixes); run_device takes what they do ask for if that is more
size_t tmp_bound(int64_t n, int64_t T) { return up256(8 * (size_t)T) + up256(4 * (size_t)T / 64) + 64 * (size_t)n + (1u << 20); }

struct Device {                     // released on every exit path (the stream has drained before the buffer is freed: dp_hip.h)
    DevBuf mem;
    Stream st;
    Event ev[5];
};

#define HIPG(x) PG_HIP_CODE(x, "pagan guide", PAGAN_E_INTERNAL)

int waves_per_pair(int64_t pairs) {
    // enough waves to fill the chip's 8,192 wave slots when the pairs alone do not (32 x 100 kb: 496 pairs)
    int w = 16;
    while (w > 1 && pairs * w > 8192) w >>= 1;
    return w;
}

// S of all pairs (row-major over x < y) and the k-mer counts, from the device
int run_device(const GuideInput &in, int n, int k, std::vector<uint32_t> *pair_sums, std::vector<uint32_t> *kmers, pagan_guide_info *info) {
    const int64_t T = (int64_t)in.letters.size(), P = (int64_t)n * (n - 1) / 2;
    int ndev = 0, device = -1;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return PAGAN_E_NODEVICE;
    if (hipGetDevice(&device) != hipSuccess) return PAGAN_E_NODEVICE;      // the caller's current device; nothing here changes it
    // (from here on a HIP error is PAGAN_E_NOMEM or PAGAN_E_INTERNAL: the device is there)
    pair_sums->assign((size_t)P, 0);
    kmers->assign((size_t)n, 0);
    info->waves_per_pair = waves_per_pair(P);
    if (T == 0) return PAGAN_OK;
    Device D;
    HIPG(D.st.create(hipStreamNonBlocking));
    for (Event &e : D.ev) HIPG(e.create());
    hipStream_t st = D.st;
    const unsigned end_bit = (unsigned)(in.bits * k + 1);
    size_t tmp_sort = 0, tmp_scan = 0;
    HIPG(rocprim::segmented_radix_sort_keys(nullptr, tmp_sort, (uint64_t *)nullptr, (uint64_t *)nullptr, (unsigned)T, (unsigned)n,
                                            (const uint32_t *)nullptr, (const uint32_t *)nullptr, 0u, end_bit, st));
    HIPG(rocprim::exclusive_scan(nullptr, tmp_scan, (uint32_t *)nullptr, (uint32_t *)nullptr, 0u, (size_t)T + 1, rocprim::plus<uint32_t>(), st));
    const Layout L(n, T, std::max(tmp_bound(n, T), std::max(tmp_sort, tmp_scan)));
    HIPG(D.mem.alloc(L.total));
    info->device_bytes = (int64_t)L.total;
    char *m = D.mem;
    unsigned char *letters = (unsigned char *)(m + L.letters);
    uint32_t *off = (uint32_t *)(m + L.off), *d_kmers = (uint32_t *)(m + L.kmers), *list_off = (uint32_t *)(m + L.list_off);
    uint64_t *keys_in = (uint64_t *)(m + L.keys_in), *keys = (uint64_t *)(m + L.keys_out), *codes = keys_in;
    uint32_t *seg = (uint32_t *)(m + L.seg), *head = (uint32_t *)(m + L.head), *pos = (uint32_t *)(m + L.pos);
    uint32_t *run_start = (uint32_t *)(m + L.run_start), *counts = (uint32_t *)(m + L.counts), *d_pairs = (uint32_t *)(m + L.pairs);
    void *tmp = m + L.tmp;
    const size_t tmp_bytes = L.total - L.tmp;
    HIPG(hipMemcpyAsync(letters, in.letters.data(), (size_t)T, hipMemcpyHostToDevice, st));
    HIPG(hipMemcpyAsync(off, in.off.data(), 4 * (size_t)(n + 1), hipMemcpyHostToDevice, st));
    const int Bk = 256;
    const unsigned g_pos = (unsigned)((std::max<int64_t>(T, n) + 1 + Bk - 1) / Bk), g_seq = (unsigned)((n + Bk - 1) / Bk);
    HIPG(hipEventRecord(D.ev[0], st));
    hipLaunchKernelGGL(pgd_pack, dim3((unsigned)((T + Bk - 1) / Bk)), dim3(Bk), 0, st, letters, (uint32_t)T, off, n, k, in.bits, keys_in, seg);
    HIPG(hipEventRecord(D.ev[1], st));
    size_t ts = tmp_bytes;
    HIPG(rocprim::segmented_radix_sort_keys(tmp, ts, keys_in, keys, (unsigned)T, (unsigned)n, off, off + 1, 0u, end_bit, st));
    HIPG(hipEventRecord(D.ev[2], st));
    hipLaunchKernelGGL(pgd_kmers, dim3(g_seq), dim3(Bk), 0, st, keys, off, n, d_kmers);
    hipLaunchKernelGGL(pgd_heads, dim3(g_pos), dim3(Bk), 0, st, keys, seg, off, (uint32_t)T, head);
    ts = tmp_bytes;
    HIPG(rocprim::exclusive_scan(tmp, ts, head, pos, 0u, (size_t)T + 1, rocprim::plus<uint32_t>(), st));
    hipLaunchKernelGGL(pgd_emit, dim3(g_pos), dim3(Bk), 0, st, keys, head, pos, off, (uint32_t)T, n, codes, run_start, list_off);
    hipLaunchKernelGGL(pgd_counts, dim3((unsigned)((T + Bk - 1) / Bk)), dim3(Bk), 0, st, run_start, seg, off, d_kmers, list_off, pos + T, (uint32_t)T, counts);
    HIPG(hipEventRecord(D.ev[3], st));
    hipLaunchKernelGGL(pgd_pairs, dim3((unsigned)std::min<uint64_t>((uint64_t)P, kMaxPairGroups)), dim3(64 * info->waves_per_pair), 0, st, codes,
                       counts, list_off, n, (uint64_t)P, d_pairs);
    HIPG(hipEventRecord(D.ev[4], st));
    HIPG(hipGetLastError());
    uint32_t n_runs = 0;
    HIPG(hipMemcpyAsync(&n_runs, pos + T, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIPG(hipMemcpyAsync(pair_sums->data(), d_pairs, 4 * (size_t)P, hipMemcpyDeviceToHost, st));
    HIPG(hipMemcpyAsync(kmers->data(), d_kmers, 4 * (size_t)n, hipMemcpyDeviceToHost, st));
    HIPG(hipStreamSynchronize(st));
    float ms[4] = {0, 0, 0, 0};
    for (int e = 0; e < 4; ++e) HIPG(hipEventElapsedTime(&ms[e], D.ev[e], D.ev[e + 1]));
    info->pack_ms = ms[0]; info->sort_ms = ms[1]; info->compress_ms = ms[2]; info->pairs_ms = ms[3];
    if (n_runs > (uint32_t)T) return PAGAN_E_INTERNAL;
    info->entries = n_runs;
    return PAGAN_OK;
}

int distances(int32_t n, const char *const *seqs, int32_t data_type, int32_t k, int64_t *shared, int64_t *kmers_out, double *dist,
              pagan_guide_info *info_out) {
    if (n < 2 || n > PAGAN_GUIDE_MAX_SEQS || !seqs || k < 0 || k > 31) return PAGAN_E_ARG;
    try {
        GuideInput in;
        const int rc = guide_clean(n, seqs, data_type, &in);
        if (rc != PAGAN_OK) return rc;
        if (k > in.max_k) return PAGAN_E_ARG;
        if (k == 0) k = pagan_guide_kmer_length(in.data_type, in.longest);
        pagan_guide_info info;
        std::memset(&info, 0, sizeof(info));
        info.k = k; info.data_type = in.data_type; info.pair_chunk = kChunk;
        info.positions = (int64_t)in.letters.size(); info.pairs = (int64_t)n * (n - 1) / 2;
        std::vector<uint32_t> sums, kmers;
        const int rd = run_device(in, n, k, &sums, &kmers, &info);
        if (rd != PAGAN_OK) return rd;
        if (kmers_out) for (int x = 0; x < n; ++x) kmers_out[x] = kmers[x];
        size_t pair = 0;
        for (int x = 0; x < n; ++x) {
            if (shared) shared[(size_t)x * n + x] = kmers[x];
            if (dist) dist[(size_t)x * n + x] = 0.0;
            for (int y = x + 1; y < n; ++y, ++pair) {
                const int64_t S = sums[pair], m = std::min(kmers[x], kmers[y]);
                if (S > m) return PAGAN_E_INTERNAL;
                if (shared) shared[(size_t)x * n + y] = shared[(size_t)y * n + x] = S;
                if (dist) dist[(size_t)x * n + y] = dist[(size_t)y * n + x] = pagan_guide_distance_of(S, m, k, in.data_type);
            }
        }
        if (info_out) *info_out = info;
        return PAGAN_OK;
    } catch (const std::bad_alloc &) {
        return PAGAN_E_NOMEM;
    }
}

} // namespace

} // namespace pagan

using namespace pagan;

extern "C" {

int pagan_guide_distances(int32_t n, const char *const *seqs, int32_t data_type, int32_t k, int64_t *shared, int64_t *kmers,
                          double *dist, pagan_guide_info *info) {
    return distances(n, seqs, data_type, k, shared, kmers, dist, info);
}

int64_t pagan_guide_tree(int32_t n, const char *const *names, const char *const *seqs, int32_t data_type, int32_t k,
                         char *newick_out, int64_t cap, pagan_guide_info *info) {
    if (n < 2 || n > PAGAN_GUIDE_MAX_SEQS || (cap > 0 && !newick_out)) return PAGAN_E_ARG;
    if (guide_check_names(n, names) != PAGAN_OK) return PAGAN_E_ARG;
    try {
        std::vector<double> dist((size_t)n * n);
        pagan_guide_info local;
        const int rc = distances(n, seqs, data_type, k, nullptr, nullptr, dist.data(), &local);
        if (rc != PAGAN_OK) return rc;
        const auto t0 = std::chrono::steady_clock::now();
        const int64_t need = pagan_guide_upgma(n, names, dist.data(), newick_out, cap);
        local.upgma_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        if (info) *info = local;
        return need;
    } catch (const std::bad_alloc &) {
        return PAGAN_E_NOMEM;
    }
}

int64_t pagan_guide_predict_bytes(int32_t n, int64_t total_len) {
    if (n < 2 || n > PAGAN_GUIDE_MAX_SEQS || total_len < 0 || total_len > PAGAN_GUIDE_MAX_POSITIONS) return PAGAN_E_ARG;
    return (int64_t)Layout(n, total_len, tmp_bound(n, total_len)).total;
}

} // extern "C"
