// dp_alndist.hip -- row pair counts of an alignment on the device, the input of the guide tree made from the alignment
// (include/pagan_host.h, "guide tree from an alignment"; DESIGN.md "Guide tree from the alignment").  For all pairs of N rows of
// L columns: both = columns where each row holds a letter, match = those of them with equal codes.
//   pad_pack    the rows arrive as bytes.  A wave takes 64 columns of a row, every lane classifies its character through a
//               256-entry table (LDS), and __ballot gives one 64-bit word per plane: `valid`, then the code's bits (2 for DNA,
//               5 for protein), 0 where valid is 0.  Layout [word][plane][row]: one word of 64 consecutive rows is 512 contiguous
//               bytes.  Rows are padded to a multiple of the tile height and words to a multiple of the split granule, all with
//               valid = 0, so that the pair kernel has no edge cases.
//   pad_pairs   a popcount "matrix product" over the upper triangle of 64 x 64 row tiles, tx <= ty.  A workgroup (four waves)
//               owns a tile, or, when the tiles alone do not fill the chip, the words [split * per, (split + 1) * per) of one.
//               A lane owns one x row and holds its planes of the current word(s) in registers.  Wave w keeps the y rows
//               16 w .. 16 w + 15, whose words are wave-uniform: one plane of the 16 rows is 128 contiguous bytes, taken with
//               scalar loads into SGPRs (staging them in LDS and reading them back as a broadcast was measured 7-10 % slower:
//               DESIGN.md).  32 uint32 accumulators a lane.  Per (x, y, word): m = valid_x & valid_y, both += popc(m),
//               match += popc(m & ~(OR of the code planes' XOR)).  Results are stored once, coalesced along x, as the tile's
//               slice [both | match][y][x].
//   pad_fold    with S > 1 splits: slice t += slices S' * tiles + t, S' = 1 .. S - 1, in that order.
// Integers only, no atomics, nothing depends on timing.  The host fills both triangles of the returned matrices from the tiles.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/pagan_host.h"
#include "dp_hip.h"
#include "host_guide.h"

namespace pagan {

using namespace pgdev;

namespace {

constexpr int kTile = PAGAN_ALN_TILE, kGranule = PAGAN_ALN_SPLIT_WORDS, kWaves = 4, kRowsPerWave = kTile / kWaves;
constexpr uint32_t kTileCounts = 2 * kTile * kTile;                  // both and match of one tile
static_assert(kTile == 64, "a lane of a wave owns an x row of the tile");
// every tile (times its splits, at most 1,024 workgroups for fewer tiles than that) is a workgroup of one launch: at the
// largest n that is 524,800, under the 2^20 workgroups dp_guide.hip caps a launch at, so no launch dimension needs a stride
static_assert((uint64_t)(PAGAN_GUIDE_MAX_SEQS / kTile) * (PAGAN_GUIDE_MAX_SEQS / kTile + 1) / 2 <= (1u << 20), "tiles of one launch");
constexpr uint64_t kMaxPackGroups = 1u << 20;

template <int P>
__global__ __launch_bounds__(256) void pad_pack(const unsigned char *__restrict__ bytes, const unsigned char *__restrict__ table, uint32_t n,
                                                uint32_t L, uint32_t rows_pad, uint32_t words_pad, uint64_t *__restrict__ packed) {
    __shared__ unsigned char tab[256];
    tab[threadIdx.x] = table[threadIdx.x];
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t items = (uint64_t)(rows_pad / kTile) * words_pad;            // (tile row, word)
    for (uint64_t it = blockIdx.x; it < items; it += gridDim.x) {
        const uint32_t tr = (uint32_t)(it / words_pad), w = (uint32_t)(it % words_pad);
        const uint32_t r0 = tr * kTile + wave * kRowsPerWave;
        const uint64_t col = (uint64_t)w * 64 + lane;
        uint64_t keep[P];                                                        // lane j: the planes of row r0 + j
#pragma unroll
        for (int p = 0; p < P; ++p) keep[p] = 0;
#pragma unroll 4
        for (uint32_t j = 0; j < (uint32_t)kRowsPerWave; ++j) {
            const uint32_t r = r0 + j;
            unsigned code = kGuideNoLetter;
            if (r < n && col < L) code = tab[bytes[(uint64_t)r * L + col]];
            const bool valid = code != kGuideNoLetter;
            uint64_t b = __ballot(valid);
            if (lane == j) keep[0] = b;
#pragma unroll
            for (int p = 1; p < P; ++p) {
                b = __ballot(valid && ((code >> (p - 1)) & 1u));
                if (lane == j) keep[p] = b;
            }
        }
        if (lane < (uint32_t)kRowsPerWave) {
#pragma unroll
            for (int p = 0; p < P; ++p) packed[((uint64_t)w * P + p) * rows_pad + r0 + lane] = keep[p];
        }
    }
}

template <int P>
__global__ __launch_bounds__(256) void pad_pairs(const uint64_t *__restrict__ packed, uint32_t rows_pad, uint32_t tiles, uint32_t splits,
                                                 uint32_t words_pad, uint32_t words_per_split, uint32_t *__restrict__ out) {
    constexpr int kWordsPerStep = P == 3 ? 2 : 1;                   // measured: two words a step win 10 % for DNA, lose 5 % for protein
    static_assert(kGranule % kWordsPerStep == 0, "a split is whole granules, so whole steps");
    const uint32_t tile = blockIdx.x / splits, split = blockIdx.x % splits;
    // tile index -> (tx, ty), tx <= ty: row tx starts at tx (2 T - tx + 1) / 2; the largest tx whose start is <= the index
    const uint64_t T = rows_pad / kTile;
    uint32_t xl = 0, xh = (uint32_t)T - 1;
    while (xl < xh) {
        const uint64_t mid = ((uint64_t)xl + xh + 1) >> 1;
        if (mid * (2 * T - mid + 1) / 2 <= tile) xl = (uint32_t)mid; else xh = (uint32_t)mid - 1;
    }
    const uint32_t tx = xl, ty = tx + (uint32_t)(tile - (uint64_t)tx * (2 * T - tx + 1) / 2);
    const uint32_t lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t w0 = split * words_per_split, w1 = min(words_pad, w0 + words_per_split);     // (whole granules)
    uint32_t both[kRowsPerWave], match[kRowsPerWave];
#pragma unroll
    for (int j = 0; j < kRowsPerWave; ++j) both[j] = match[j] = 0;
    const uint64_t *xp = packed + (uint64_t)tx * kTile + lane;
    const uint64_t *yp = packed + (uint64_t)ty * kTile + wave * kRowsPerWave;       // the same address in every lane: scalar loads
    for (uint32_t w = w0; w < w1; w += kWordsPerStep) {
        uint64_t xv[kWordsPerStep][P];
#pragma unroll
        for (int u = 0; u < kWordsPerStep; ++u)
#pragma unroll
            for (int p = 0; p < P; ++p) xv[u][p] = xp[((uint64_t)(w + u) * P + p) * rows_pad];
#pragma unroll
        for (int u = 0; u < kWordsPerStep; ++u)
#pragma unroll
            for (int j = 0; j < kRowsPerWave; ++j) {
                const uint64_t m = xv[u][0] & yp[((uint64_t)(w + u) * P) * rows_pad + j];
                uint64_t diff = 0;
#pragma unroll
                for (int p = 1; p < P; ++p) diff |= xv[u][p] ^ yp[((uint64_t)(w + u) * P + p) * rows_pad + j];
                both[j] += (uint32_t)__popcll(m);
                match[j] += (uint32_t)__popcll(m & ~diff);
            }
    }
    uint32_t *o = out + ((uint64_t)split * tiles + tile) * kTileCounts + (wave * kRowsPerWave) * kTile + lane;
#pragma unroll
    for (int j = 0; j < kRowsPerWave; ++j) {
        o[j * kTile] = both[j];
        o[kTile * kTile + j * kTile] = match[j];
    }
}

__global__ __launch_bounds__(256) void pad_fold(uint32_t *__restrict__ out, uint32_t tiles, uint32_t splits) {
    const uint64_t per = (uint64_t)tiles * kTileCounts, i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= per) return;
    uint32_t sum = out[i];
    for (uint32_t s = 1; s < splits; ++s) sum += out[(uint64_t)s * per + i];
    out[i] = sum;
}

struct Device {                     // released on every exit path (the stream has drained before the buffer is freed: dp_hip.h)
    DevBuf mem;
    Stream st;
    Event ev[3];
};

#define HIPA(x) PG_HIP_CODE(x, "pagan aln", PAGAN_E_INTERNAL)

// the tiles' counts [tiles][both | match][y][x] from the device
int run_device(int n, const char *const *rows, int64_t columns, int planes, int data_type, std::vector<uint32_t> *counts, pagan_aln_info *info) {
    int ndev = 0, device = -1;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return PAGAN_E_NODEVICE;
    if (hipGetDevice(&device) != hipSuccess) return PAGAN_E_NODEVICE;      // the caller's current device; nothing here changes it
    const AlnLayout L(n, columns, planes);
    info->col_splits = L.splits;
    info->device_bytes = (int64_t)L.total;
    counts->assign((size_t)L.tiles * kTileCounts, 0);
    std::vector<unsigned char> bytes((size_t)n * (size_t)columns);
    for (int r = 0; r < n; ++r) if (columns) std::memcpy(bytes.data() + (size_t)r * (size_t)columns, rows[r], (size_t)columns);
    unsigned char table[256];
    aln_letter_table(data_type, table);
    Device D;
    HIPA(D.st.create(hipStreamNonBlocking));
    for (Event &e : D.ev) HIPA(e.create());
    hipStream_t st = D.st;
    HIPA(D.mem.alloc(L.total));
    unsigned char *d_bytes = (unsigned char *)(D.mem.h + L.bytes), *d_table = (unsigned char *)(D.mem.h + L.table);
    uint64_t *packed = (uint64_t *)(D.mem.h + L.packed);
    uint32_t *out = (uint32_t *)(D.mem.h + L.out);
    if (!bytes.empty()) HIPA(hipMemcpyAsync(d_bytes, bytes.data(), bytes.size(), hipMemcpyHostToDevice, st));
    HIPA(hipMemcpyAsync(d_table, table, 256, hipMemcpyHostToDevice, st));
    const uint32_t rows_pad = (uint32_t)L.rows_pad, words_pad = (uint32_t)L.words_pad, tiles = (uint32_t)L.tiles, splits = (uint32_t)L.splits;
    const uint32_t granules = words_pad / kGranule, per = (granules + splits - 1) / splits * kGranule;
    const uint64_t items = (uint64_t)(rows_pad / kTile) * words_pad;
    HIPA(hipEventRecord(D.ev[0], st));
    if (items) {
        const dim3 g((unsigned)std::min<uint64_t>(items, kMaxPackGroups));
        if (planes == 3) hipLaunchKernelGGL(pad_pack<3>, g, dim3(256), 0, st, d_bytes, d_table, (uint32_t)n, (uint32_t)columns, rows_pad, words_pad, packed);
        else hipLaunchKernelGGL(pad_pack<6>, g, dim3(256), 0, st, d_bytes, d_table, (uint32_t)n, (uint32_t)columns, rows_pad, words_pad, packed);
    }
    HIPA(hipEventRecord(D.ev[1], st));
    if (planes == 3) hipLaunchKernelGGL(pad_pairs<3>, dim3(tiles * splits), dim3(256), 0, st, packed, rows_pad, tiles, splits, words_pad, per, out);
    else hipLaunchKernelGGL(pad_pairs<6>, dim3(tiles * splits), dim3(256), 0, st, packed, rows_pad, tiles, splits, words_pad, per, out);
    if (splits > 1)
        hipLaunchKernelGGL(pad_fold, dim3((unsigned)(((uint64_t)tiles * kTileCounts + 255) / 256)), dim3(256), 0, st, out, tiles, splits);
    HIPA(hipEventRecord(D.ev[2], st));
    HIPA(hipGetLastError());
    HIPA(hipMemcpyAsync(counts->data(), out, counts->size() * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIPA(hipStreamSynchronize(st));
    float ms[2] = {0, 0};
    for (int e = 0; e < 2; ++e) HIPA(hipEventElapsedTime(&ms[e], D.ev[e], D.ev[e + 1]));
    info->pack_ms = ms[0]; info->pairs_ms = ms[1];
    return PAGAN_OK;
}

int distances(int32_t n, const char *const *rows, int32_t data_type, int64_t *both, int64_t *match, double *dist, pagan_aln_info *info_out) {
    int64_t columns = 0;
    int type = 0;
    try {
        const int rc = aln_check_rows(n, rows, data_type, &columns, &type);
        if (rc != PAGAN_OK) return rc;
        pagan_aln_info info;
        std::memset(&info, 0, sizeof(info));
        info.data_type = type; info.planes = type == 2 ? 6 : 3; info.tile = kTile;
        info.columns = columns; info.words = (columns + 63) / 64; info.pairs = (int64_t)n * (n - 1) / 2;
        std::vector<uint32_t> counts;
        const int rd = run_device(n, rows, columns, info.planes, type, &counts, &info);
        if (rd != PAGAN_OK) return rd;
        const size_t N = (size_t)n, T = (N + kTile - 1) / kTile;
        size_t tile = 0;
        for (size_t tx = 0; tx < T; ++tx)
            for (size_t ty = tx; ty < T; ++ty, ++tile) {
                const uint32_t *b = counts.data() + tile * kTileCounts, *m = b + kTile * kTile;
                for (size_t yl = 0; yl < (size_t)kTile && ty * kTile + yl < N; ++yl)
                    for (size_t xl = 0; xl < (size_t)kTile && tx * kTile + xl < N; ++xl) {
                        const size_t x = tx * kTile + xl, y = ty * kTile + yl;
                        const int64_t vb = b[yl * kTile + xl], vm = m[yl * kTile + xl];
                        if (vm > vb || vb > columns) return PAGAN_E_INTERNAL;
                        if (both) both[x * N + y] = both[y * N + x] = vb;
                        if (match) match[x * N + y] = match[y * N + x] = vm;
                        if (dist) dist[x * N + y] = dist[y * N + x] = x == y ? 0.0 : pagan_guide_distance_of(vm, vb, 1, type);
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

int pagan_aln_distances(int32_t n, const char *const *rows, int32_t data_type, int64_t *both, int64_t *match, double *dist,
                        pagan_aln_info *info) {
    return distances(n, rows, data_type, both, match, dist, info);
}

int64_t pagan_aln_tree(int32_t n, const char *const *names, const char *const *rows, int32_t data_type, char *newick_out, int64_t cap,
                       pagan_aln_info *info) {
    if (n < 2 || n > PAGAN_GUIDE_MAX_SEQS || (cap > 0 && !newick_out)) return PAGAN_E_ARG;
    if (guide_check_names(n, names) != PAGAN_OK) return PAGAN_E_ARG;
    try {
        std::vector<double> dist((size_t)n * n);
        pagan_aln_info local;
        const int rc = distances(n, rows, data_type, nullptr, nullptr, dist.data(), &local);
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

} // extern "C"
