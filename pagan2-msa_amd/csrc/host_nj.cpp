// host_nj.cpp -- the host side of neighbour joining (include/pagan_host.h, "neighbour joining"): the input's checks, the device
// buffers' layout, and what turns the joins the device made into a tree the walk can take -- the clamp, the midpoint rooting and
// the Newick string.  Nothing here needs a device: tests/test_nj_cpu.py feeds pagan_nj_newick with the joins of the second reading.
//
// The rooting works on the tree as the joins hang it, from the star node: cluster ids grow towards the star, so one pass in id
// order has every child before its parent.  Putting the root on the edge above c then only turns round the edges on the path
// from c's parent up to the star; every other node keeps its parent.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "../../include/pagan_host.h"
#include "dp_pool.h"
#include "host_guide.h"
#include "host_nj.h"

namespace pagan {

NjLayout::NjLayout(int64_t n) {
    pgdev::Carve c{nullptr};
    matrix = c.skip((size_t)n * (size_t)n * sizeof(double));
    R = c.skip((size_t)n * sizeof(double));
    id = c.skip((size_t)n * sizeof(int32_t));
    best = c.skip((size_t)n * sizeof(NjRowBest));
    cur = c.skip(sizeof(NjPick));
    log = c.skip((size_t)(n - 3) * sizeof(NjRecord) + sizeof(NjStar));
    total = c.cur;
}

int nj_check_input(int32_t n, const double *dist) {
    if (n < 2 || n > PAGAN_NJ_MAX_SEQS || !dist) return PAGAN_E_ARG;
    for (int i = 0; i < n; ++i)
        for (int j = i + 1; j < n; ++j) {
            const double v = dist[(size_t)i * n + j];
            if (!std::isfinite(v) || v < 0) return PAGAN_E_ARG;
        }
    return PAGAN_OK;
}

namespace {

int64_t hand_out(const std::string &out, char *newick_out, int64_t cap) {
    const int64_t need = (int64_t)out.size() + 1;
    if (need <= cap) std::memcpy(newick_out, out.c_str(), (size_t)need);
    return need;
}

double clamped(double len) { return len > 0 ? len : 0.0; }

} // namespace

} // namespace pagan

using namespace pagan;

extern "C" {

int64_t pagan_nj_predict_bytes(int32_t n) {
    if (n < 2 || n > PAGAN_NJ_MAX_SEQS) return PAGAN_E_ARG;
    return n == 2 ? 0 : (int64_t)NjLayout(n).total;
}

int64_t pagan_nj_newick(int32_t n, const char *const *names, const int32_t *join_ids, const double *join_len,
                        const int32_t star_ids[3], const double star_len[3], char *newick_out, int64_t cap) {
    if (n < 2 || n > PAGAN_NJ_MAX_SEQS || !star_ids || !star_len || (cap > 0 && !newick_out)) return PAGAN_E_ARG;
    if (n > 3 && (!join_ids || !join_len)) return PAGAN_E_ARG;
    if (guide_check_names(n, names) != PAGAN_OK) return PAGAN_E_ARG;
    try {
        char num[40];
        if (n == 2) {
            if (star_ids[0] != 0 || star_ids[1] != 1 || !std::isfinite(star_len[0]) || !std::isfinite(star_len[1])) return PAGAN_E_ARG;
            std::string out = "(";
            for (int k = 0; k < 2; ++k) {
                out += names[k];
                std::snprintf(num, sizeof(num), ":%.17g", clamped(star_len[k]));
                out += num;
                out += k == 0 ? ',' : ')';
            }
            out += ';';
            return hand_out(out, newick_out, cap);
        }
        // the tree as the joins hang it: nodes 0 .. 2n-3, the star 2n-3; the root to come is 2n-2
        const int joins = n - 3, star = 2 * n - 3, root = 2 * n - 2;
        std::vector<int> parent((size_t)root + 1, -1);
        std::vector<double> len((size_t)root + 1, 0.0);
        std::vector<char> active((size_t)star, 0);
        std::fill(active.begin(), active.begin() + n, 1);
        auto hang = [&](int child, int above, double raw) {
            if (child < 0 || child >= above || !active[child] || !std::isfinite(raw)) return false;
            active[child] = 0; parent[child] = above; len[child] = clamped(raw);
            return true;
        };
        for (int t = 0; t < joins; ++t) {
            const int i = join_ids[2 * t], j = join_ids[2 * t + 1], u = n + t;
            if (i >= j || !hang(i, u, join_len[2 * t]) || !hang(j, u, join_len[2 * t + 1])) return PAGAN_E_ARG;
            active[u] = 1;
        }
        if (star_ids[0] >= star_ids[1] || star_ids[1] >= star_ids[2]) return PAGAN_E_ARG;
        for (int k = 0; k < 3; ++k)
            if (!hang(star_ids[k], star, star_len[k])) return PAGAN_E_ARG;
        // low, then every node's children in ascending low (leaf sets are disjoint: no two are equal)
        std::vector<std::vector<int>> kids((size_t)root + 1);
        std::vector<int> low((size_t)root + 1);
        auto by_low = [&](int a, int b) { return low[a] < low[b]; };
        for (int v = 0; v < star; ++v) kids[parent[v]].push_back(v);
        for (int v = 0; v <= star; ++v) {
            if (v < n) { low[v] = v; continue; }
            low[v] = low[kids[v][0]];
            for (int c : kids[v]) low[v] = std::min(low[v], low[c]);
            std::sort(kids[v].begin(), kids[v].end(), by_low);
        }
        // far, the child of the largest offer, span; the top node
        std::vector<double> far((size_t)star + 1, 0.0), span((size_t)star + 1, 0.0);
        std::vector<int> toward((size_t)star + 1, -1);
        int top = -1;
        for (int v = n; v <= star; ++v) {
            double first = 0, second = 0;
            int c1 = -1, c2 = -1;
            for (int c : kids[v]) {
                const double offer = far[c] + len[c];
                if (c1 < 0 || offer > first) { first = offer; c1 = c; }
            }
            for (int c : kids[v]) {
                if (c == c1) continue;
                const double offer = far[c] + len[c];
                if (c2 < 0 || offer > second) { second = offer; c2 = c; }
            }
            far[v] = first; toward[v] = c1; span[v] = first + second;
            if (top < 0 || span[v] > span[top]) top = v;
        }
        const double half = span[top] / 2;
        int c = toward[top];
        while (far[c] > half) c = toward[c];                             // (a leaf's far is 0 <= half)
        const double below = std::min(std::max(half - far[c], 0.0), len[c]), above = len[c] - below;
        // the root on the edge above c; the edges from c's parent up to the star turn round
        int v = parent[c], from = root;
        double carry = above;
        parent[c] = root; len[c] = below;
        while (v >= 0) {
            const int up = parent[v];
            const double up_len = len[v];
            parent[v] = from; len[v] = carry;
            from = v; carry = up_len; v = up;
        }
        // the rooted tree: children before their parents by a walk from the root, low again, the left child the smaller low
        for (auto &k : kids) k.clear();
        for (int x = 0; x < root; ++x) kids[parent[x]].push_back(x);
        std::vector<int> order;
        order.reserve((size_t)root + 1);
        order.push_back(root);
        for (size_t at = 0; at < order.size(); ++at)
            for (int k : kids[order[at]]) order.push_back(k);
        if ((int)order.size() != root + 1) return PAGAN_E_INTERNAL;
        for (size_t at = order.size(); at-- > 0;) {
            const int x = order[at];
            if (x < n) { low[x] = x; continue; }
            if (kids[x].size() != 2) return PAGAN_E_INTERNAL;
            if (low[kids[x][1]] < low[kids[x][0]]) std::swap(kids[x][0], kids[x][1]);
            low[x] = low[kids[x][0]];
        }
        std::string out;
        std::vector<std::pair<int, int>> stack;                          // (node, stage)
        stack.emplace_back(root, 0);
        while (!stack.empty()) {
            const int x = stack.back().first, stage = stack.back().second;
            if (x < n) {
                out += names[x];
                stack.pop_back();
            } else if (stage < 2) {
                out += stage == 0 ? '(' : ',';
                stack.back().second = stage + 1;
                stack.emplace_back(kids[x][stage], 0);
                continue;
            } else {
                out += ')';
                stack.pop_back();
            }
            if (x != root) {
                std::snprintf(num, sizeof(num), ":%.17g", len[x]);
                out += num;
            }
        }
        out += ';';
        return hand_out(out, newick_out, cap);
    } catch (const std::bad_alloc &) {
        return PAGAN_E_NOMEM;
    }
}

int64_t pagan_nj_tree(int32_t n, const char *const *names, const double *dist, char *newick_out, int64_t cap, pagan_nj_info *info) {
    if (nj_check_input(n, dist) != PAGAN_OK || (cap > 0 && !newick_out)) return PAGAN_E_ARG;
    if (guide_check_names(n, names) != PAGAN_OK) return PAGAN_E_ARG;
    try {
        const size_t joins = n > 3 ? (size_t)n - 3 : 0;
        std::vector<int32_t> ids(2 * joins + 1);
        std::vector<double> lens(2 * joins + 1);
        int32_t star_ids[3];
        double star_len[3];
        pagan_nj_info local;
        const int rc = pagan_nj_joins(n, dist, ids.data(), lens.data(), star_ids, star_len, &local);
        if (rc != PAGAN_OK) return rc;
        const auto t0 = std::chrono::steady_clock::now();
        const int64_t need = pagan_nj_newick(n, names, ids.data(), lens.data(), star_ids, star_len, newick_out, cap);
        local.root_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        if (info) *info = local;
        return need;
    } catch (const std::bad_alloc &) {
        return PAGAN_E_NOMEM;
    }
}

} // extern "C"
