// host_guide.cpp -- the host side of the guide tree from sequences alone (include/pagan_host.h, "guide tree"): the cleaning
// the walk applies to its input, the default k, the distance from the integers the device counted, and UPGMA -- and of the
// guide tree from an alignment (csrc/dp_alndist.hip): the rows' checks, the letter table, the split rule and the buffer layout.
//
// UPGMA keeps, for every active cluster, the partner of smallest distance over its whole row (ties: the partner of lowest id).
// The pair a step merges is the best (distance, lower id, higher id) over these row candidates: the merged pair (a, b), a < b,
// is row a's candidate -- a partner c < a at the same distance would make (c, a) the smaller pair -- so the rule "smallest
// distance, lowest first id, lowest second id" is what the scan over rows finds.  A merge writes the new cluster's row (O(N)),
// offers the new cluster to every other row (it has the highest id, so it wins no tie) and rescans only the rows whose partner
// was one of the two merged clusters: O(N) a step unless many rows pointed at the pair.
#include <algorithm>
#include <cctype>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <new>
#include <string>
#include <vector>

#include "../../include/pagan_host.h"
#include "dp_pool.h"
#include "host_guide.h"
#include "host_model.h"

namespace pagan {

int guide_clean(int32_t n, const char *const *seqs, int32_t data_type, GuideInput *out) {
    if (n < 1 || !seqs || data_type < 0 || data_type > 3) return PAGAN_E_ARG;
    std::vector<std::string> s(n);
    for (int k = 0; k < n; ++k) {
        if (!seqs[k]) return PAGAN_E_ARG;
        s[k].reserve(std::strlen(seqs[k]));
        for (const char *p = seqs[k]; *p; ++p) {                       // host_tree.cpp, pagan_msa_create: upper case, no gaps, no line ends
            const char c = (char)std::toupper((unsigned char)*p);
            if (c != '-' && c != '\r' && c != '\n') s[k].push_back(c);
        }
    }
    const int type = data_type == 1 ? kDna : data_type == 2 ? kProtein : data_type == 3 ? kCodon : ModelFactory::guess_type(s);
    out->data_type = type == kDna ? 1 : type == kProtein ? 2 : 3;
    const bool protein = type == kProtein;
    out->bits = protein ? 5 : 2;
    out->max_k = protein ? 12 : 31;
    // what the walk keeps (the full alphabet, U -> T resp. U, X -> X) and, of that, the core letters' codes
    unsigned char code[256];
    bool keep[256];
    std::memset(code, kGuideNoLetter, sizeof(code));
    std::memset(keep, 0, sizeof(keep));
    for (const char *p = protein ? ModelFactory::protein_alphabet() : ModelFactory::dna_full_alphabet(); *p; ++p) keep[(unsigned char)*p] = true;
    keep[(unsigned char)'U'] = true;
    if (protein) keep[(unsigned char)'X'] = true;
    const char *core = protein ? ModelFactory::protein_alphabet() : "ACGT";
    for (int c = 0; core[c]; ++c) code[(unsigned char)core[c]] = (unsigned char)c;
    if (!protein) code[(unsigned char)'U'] = code[(unsigned char)'T'];
    int64_t total = 0;
    out->off.assign((size_t)n + 1, 0);
    out->longest = 0;
    std::vector<int64_t> len(n, 0);
    for (int k = 0; k < n; ++k) {
        for (char c : s[k]) len[k] += keep[(unsigned char)c];
        total += len[k];
        out->longest = std::max(out->longest, len[k]);
        if (total > PAGAN_GUIDE_MAX_POSITIONS) return PAGAN_E_ARG;
        out->off[k + 1] = (uint32_t)total;
    }
    out->letters.resize((size_t)total);
    size_t w = 0;
    for (int k = 0; k < n; ++k)
        for (char c : s[k]) if (keep[(unsigned char)c]) out->letters[w++] = code[(unsigned char)c];
    return PAGAN_OK;
}

int guide_check_names(int32_t n, const char *const *names) {
    if (n < 1 || !names) return PAGAN_E_ARG;
    for (int k = 0; k < n; ++k) {
        if (!names[k] || !names[k][0]) return PAGAN_E_ARG;
        for (const char *p = names[k]; *p; ++p)
            if (std::strchr("(),:;", *p) || std::isspace((unsigned char)*p)) return PAGAN_E_ARG;
    }
    return PAGAN_OK;
}

int aln_check_rows(int32_t n, const char *const *rows, int32_t data_type, int64_t *columns, int *resolved_type) {
    if (n < 2 || n > PAGAN_GUIDE_MAX_SEQS || !rows || data_type < 0 || data_type > 3) return PAGAN_E_ARG;
    if (!rows[0]) return PAGAN_E_ARG;
    const size_t L = std::strlen(rows[0]);
    if (L >= ((size_t)1 << 31)) return PAGAN_E_ARG;
    for (int k = 1; k < n; ++k)
        if (!rows[k] || std::strlen(rows[k]) != L) return PAGAN_E_ARG;
    *columns = (int64_t)L;
    if (data_type != 0) { *resolved_type = data_type; return PAGAN_OK; }
    std::vector<std::string> s(n);                                     // guide_clean's first step: upper case, no gaps, no line ends
    for (int k = 0; k < n; ++k) {
        s[k].reserve(L);
        for (const char *p = rows[k]; *p; ++p) {
            const char c = (char)std::toupper((unsigned char)*p);
            if (c != '-' && c != '\r' && c != '\n') s[k].push_back(c);
        }
    }
    const int type = ModelFactory::guess_type(s);
    *resolved_type = type == kDna ? 1 : type == kProtein ? 2 : 3;
    return PAGAN_OK;
}

void aln_letter_table(int data_type, unsigned char table[256]) {
    std::memset(table, kGuideNoLetter, 256);
    const bool protein = data_type == 2;
    const char *core = protein ? ModelFactory::protein_alphabet() : "ACGT";
    for (int c = 0; core[c]; ++c) {
        table[(unsigned char)core[c]] = (unsigned char)c;
        table[(unsigned char)std::tolower((unsigned char)core[c])] = (unsigned char)c;
    }
    if (!protein) table[(unsigned char)'U'] = table[(unsigned char)'u'] = table[(unsigned char)'T'];
}

int aln_col_splits(int64_t tiles, int64_t words) {
    // a workgroup is four waves: 1,024 of them are four waves on every SIMD of the chip's 256 compute units.  Fewer tiles than
    // that (32 x 150,000 columns is one tile) share their words in whole granules, no split left empty.
    const int64_t target = 1024, granules = (words + PAGAN_ALN_SPLIT_WORDS - 1) / PAGAN_ALN_SPLIT_WORDS;
    if (tiles >= target || granules <= 1) return 1;
    const int64_t want = std::max<int64_t>(1, std::min(granules, target / tiles)), per = (granules + want - 1) / want;
    return (int)((granules + per - 1) / per);                          // (<= want: splits x tiles <= target)
}

AlnLayout::AlnLayout(int64_t n, int64_t columns, int planes_) {
    rows_pad = (n + PAGAN_ALN_TILE - 1) / PAGAN_ALN_TILE * PAGAN_ALN_TILE;
    const int64_t T = rows_pad / PAGAN_ALN_TILE;
    tiles = T * (T + 1) / 2;
    words = (columns + 63) / 64;
    words_pad = (words + PAGAN_ALN_SPLIT_WORDS - 1) / PAGAN_ALN_SPLIT_WORDS * PAGAN_ALN_SPLIT_WORDS;
    planes = planes_;
    splits = aln_col_splits(tiles, words);
    const size_t tile_bytes = 2 * (size_t)PAGAN_ALN_TILE * PAGAN_ALN_TILE * sizeof(uint32_t);      // both and match
    pgdev::Carve c{nullptr};                                           // (offsets: an array of no bytes takes none)
    bytes = c.skip((size_t)n * (size_t)columns);
    table = c.skip(256);
    packed = c.skip((size_t)words_pad * (size_t)planes * (size_t)rows_pad * sizeof(uint64_t));
    // slices of one tile's counts: split s of tile t writes slice s * tiles + t, and the fold adds them into slice t.  Room for
    // every S the split rule can choose at this size (S x tiles <= 1,024, S <= granules), so that the size grows with n and L
    const int64_t granules = words_pad / PAGAN_ALN_SPLIT_WORDS;
    slices = tiles >= 1024 || granules <= 1 ? tiles : std::min<int64_t>(1024, granules * tiles);
    out = c.skip((size_t)slices * tile_bytes);
    total = c.cur;
}

namespace {

struct Upgma {
    int n;
    std::vector<double> d;           // [n * n] by slot, symmetric
    std::vector<int> id, size, nn;   // per slot: cluster id, leaves, the slot of the row's best partner (-1: none)
    std::vector<char> active;
    std::vector<double> height;      // per slot
    // is partner slot j better than slot b for row i?  smaller distance, then lower id
    bool better(int i, int j, int b) const {
        if (b < 0) return true;
        const double dj = d[(size_t)i * n + j], db = d[(size_t)i * n + b];
        return dj < db || (dj == db && id[j] < id[b]);
    }
    void rescan(int i) {
        int b = -1;
        for (int j = 0; j < n; ++j) if (j != i && active[j] && better(i, j, b)) b = j;
        nn[i] = b;
    }
};

} // namespace

} // namespace pagan

using namespace pagan;

extern "C" {

int pagan_guide_kmer_length(int32_t data_type, int64_t max_len) {
    if (data_type < 1 || data_type > 3 || max_len < 0) return PAGAN_E_ARG;
    const int A = data_type == 2 ? 20 : 4, lo = data_type == 2 ? 3 : 8, hi = data_type == 2 ? 12 : 31;
    // A^k >= 16 max_len in integers: 128 bits hold 20^12 and 16 * 2^63
    const unsigned __int128 want = (unsigned __int128)16 * (unsigned __int128)max_len;
    unsigned __int128 pw = 1;
    int k = 0;
    while (pw < want && k < hi) { pw *= (unsigned)A; ++k; }
    return std::max(lo, std::min(hi, k));
}

double pagan_guide_distance_of(int64_t shared, int64_t m, int32_t k, int32_t data_type) {
    const double nan = std::numeric_limits<double>::quiet_NaN();
    if (data_type < 1 || data_type > 3 || k < 1 || k > (data_type == 2 ? 12 : 31) || shared < 0 || m < 0 || shared > m) return nan;
    const double F = m > 0 ? (double)shared / (double)m : 0.0;
    double p = F > 0 ? 1.0 - std::pow(F, 1.0 / (double)k) : 1.0;
    if (p <= 0) return 0.0;
    if (data_type == 2) {
        if (p > 0.85) p = 0.85;
        return -std::log(1.0 - p - 0.2 * p * p);
    }
    if (p > 0.7) p = 0.7;
    return -0.75 * std::log(1.0 - p / 0.75);
}

int64_t pagan_aln_predict_bytes(int32_t n, int64_t columns) {
    if (n < 2 || n > PAGAN_GUIDE_MAX_SEQS || columns < 0 || columns >= ((int64_t)1 << 31)) return PAGAN_E_ARG;
    return (int64_t)AlnLayout(n, columns, 6).total;
}

int64_t pagan_guide_upgma(int32_t n, const char *const *names, const double *dist, char *newick_out, int64_t cap) {
    if (n < 2 || n > PAGAN_GUIDE_MAX_SEQS || !dist || (cap > 0 && !newick_out)) return PAGAN_E_ARG;
    if (guide_check_names(n, names) != PAGAN_OK) return PAGAN_E_ARG;
    for (int i = 0; i < n; ++i)
        for (int j = i + 1; j < n; ++j) {
            const double v = dist[(size_t)i * n + j];
            if (!std::isfinite(v) || v < 0) return PAGAN_E_ARG;
        }
    try {
        Upgma u;
        u.n = n;
        u.d.assign((size_t)n * n, 0.0);
        for (int i = 0; i < n; ++i)
            for (int j = i + 1; j < n; ++j) u.d[(size_t)i * n + j] = u.d[(size_t)j * n + i] = dist[(size_t)i * n + j];
        u.id.resize(n); u.size.assign(n, 1); u.nn.assign(n, -1); u.active.assign(n, 1); u.height.assign(n, 0.0);
        for (int i = 0; i < n; ++i) u.id[i] = i;
        for (int i = 0; i < n; ++i) u.rescan(i);
        // the tree: node ids are cluster ids
        std::vector<int> left(2 * (size_t)n - 1, -1), right(2 * (size_t)n - 1, -1);
        std::vector<double> branch(2 * (size_t)n - 1, 0.0);
        for (int t = 0; t < n - 1; ++t) {
            int sa = -1, sb = -1;                                        // slots of the pair, id[sa] < id[sb]
            double best = 0;
            for (int i = 0; i < n; ++i) {
                if (!u.active[i] || u.nn[i] < 0) continue;
                int a = i, b = u.nn[i];
                if (u.id[a] > u.id[b]) std::swap(a, b);
                const double v = u.d[(size_t)a * n + b];
                if (sa < 0 || v < best || (v == best && (u.id[a] < u.id[sa] || (u.id[a] == u.id[sa] && u.id[b] < u.id[sb])))) { sa = a; sb = b; best = v; }
            }
            const int node = n + t;
            const double h = best / 2;
            left[node] = u.id[sa]; right[node] = u.id[sb];
            const double bl = h - u.height[sa], br = h - u.height[sb];
            branch[u.id[sa]] = bl > 0 ? bl : 0.0;
            branch[u.id[sb]] = br > 0 ? br : 0.0;
            const double na = (double)u.size[sa], nb = (double)u.size[sb];
            u.active[sb] = 0;
            for (int c = 0; c < n; ++c) {
                if (!u.active[c] || c == sa) continue;
                const double v = (na * u.d[(size_t)sa * n + c] + nb * u.d[(size_t)sb * n + c]) / (na + nb);
                u.d[(size_t)sa * n + c] = u.d[(size_t)c * n + sa] = v;
            }
            u.id[sa] = node; u.size[sa] += u.size[sb]; u.height[sa] = h;
            u.rescan(sa);
            for (int c = 0; c < n; ++c) {
                if (!u.active[c] || c == sa) continue;
                // (a row that pointed at either merged cluster: slot sa now holds the new cluster with another distance)
                if (u.nn[c] == sa || u.nn[c] == sb) u.rescan(c);
                else if (u.better(c, sa, u.nn[c])) u.nn[c] = sa;
            }
        }
        // Newick, children before their parent, without recursion
        std::string out;
        std::vector<std::pair<int, int>> stack;                          // (node, stage)
        stack.emplace_back(2 * n - 2, 0);
        char num[40];
        while (!stack.empty()) {
            const int v = stack.back().first, stage = stack.back().second;
            if (left[v] < 0) {
                out += names[v];
                stack.pop_back();
            } else if (stage == 0) {
                out += '(';
                stack.back().second = 1;
                stack.emplace_back(left[v], 0);
                continue;
            } else if (stage == 1) {
                out += ',';
                stack.back().second = 2;
                stack.emplace_back(right[v], 0);
                continue;
            } else {
                out += ')';
                stack.pop_back();
            }
            if (v != 2 * n - 2) {
                std::snprintf(num, sizeof(num), ":%.17g", branch[v]);
                out += num;
            }
        }
        out += ';';
        const int64_t need = (int64_t)out.size() + 1;
        if (need <= cap) std::memcpy(newick_out, out.c_str(), (size_t)need);
        return need;
    } catch (const std::bad_alloc &) {
        return PAGAN_E_NOMEM;
    }
}

} // extern "C"
