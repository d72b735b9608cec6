// fb_plan_main.cpp -- the forward/backward planner (pagan2-msa_amd/csrc/dp_fb_plan.cpp) on its own, for a host compiler's
// sanitizers: tests/test_fb_plan_cpu.py compiles this file with dp_fb_plan.cpp under -fsanitize=address,undefined, writes the
// pairs, the environments and the caps of tests/fb_plan_cases.py into a text file, runs the program on it as a child process and
// compares what it prints with what the library's exports answer.
//
// Input, whitespace-separated: the caps (count, then forward / backward pairs), the environments (count; each: count, then name
// value pairs), the pairs (count; each: name, left graph, right graph, band).  A graph: n_sites n_edges n_bwd, then state
// [n_sites], bwd_off [n_sites + 1], bwd_src, bwd_eid [n_bwd], bwd_logw [n_bwd] as the floats' bits.  A band: n (0: none),
// upper [n], lower [n].
// Output: "ladder <width> <rows> <threads>" for fb_block_for about its steps, per environment a line "switches <env> ..." with
// FbSwitches' fields in their order, per environment and pair a line "plan <env> <pair> ..." (the Python test has the format).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <set>
#include <string>
#include <utility>
#include <vector>

#include "../../pagan2-msa_amd/csrc/dp_fb_plan.h"

// pagan_fb_predict_bytes asks dp_plan.cpp for this; the program plans pairs and predicts nothing
extern "C" int64_t pagan_dp_count_cells(int32_t, int32_t, const pagan_band *) { return PAGAN_E_ARG; }

namespace {

struct Graph {
    std::vector<int32_t> state, off, src, eid;
    std::vector<float> logw;
    pagan_graph g{};
    void read(std::istream &in) {
        int n_sites = 0, n_edges = 0, nb = 0;
        in >> n_sites >> n_edges >> nb;
        state.resize(n_sites); off.resize(n_sites + 1); src.resize(nb); eid.resize(nb); logw.resize(nb);
        for (auto &v : state) in >> v;
        for (auto &v : off) in >> v;
        for (auto &v : src) in >> v;
        for (auto &v : eid) in >> v;
        for (auto &v : logw) { uint32_t bits = 0; in >> bits; std::memcpy(&v, &bits, 4); }
        g.n_sites = n_sites; g.n_edges = n_edges;
        g.state = state.data(); g.bwd_off = off.data(); g.bwd_src = src.data(); g.bwd_logw = logw.data(); g.bwd_eid = eid.data();
    }
};

struct Pair {
    std::string name;
    Graph left, right;
    std::vector<int32_t> upper, lower;
    pagan_band band{};
    void read(std::istream &in) {
        in >> name;
        left.read(in); right.read(in);
        int n = 0;
        in >> n;
        upper.resize(n); lower.resize(n);
        for (auto &v : upper) in >> v;
        for (auto &v : lower) in >> v;
        band.n = n; band.upper = upper.data(); band.lower = lower.data();
    }
};

template <class V> void print_all(const V &v) { for (auto x : v) std::printf(" %lld", (long long)x); }

} // namespace

int main(int argc, char **argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: fb_plan_main FILE\n"); return 2; }
    std::ifstream in(argv[1]);
    int n = 0;
    in >> n;
    std::vector<std::pair<int, int>> caps(n);
    for (auto &c : caps) in >> c.first >> c.second;
    in >> n;
    std::vector<std::vector<std::pair<std::string, std::string>>> envs(n);
    std::set<std::string> names;
    for (auto &env : envs) {
        in >> n;
        env.resize(n);
        for (auto &kv : env) { in >> kv.first >> kv.second; names.insert(kv.first); }
    }
    in >> n;
    std::vector<Pair> pairs(n);
    for (Pair &p : pairs) p.read(in);
    if (!in) { std::fprintf(stderr, "fb_plan_main: %s is cut short\n", argv[1]); return 2; }

    // the ladder about every width at which either form steps up
    for (int rung : {64, 96, 128, 192, 256, 384, 512, 768, 1024})
        for (int w = rung - 1; w <= rung + 1; ++w) std::printf("ladder %d %d %d\n", w, fbplan::fb_block_for(w), fbplan::fb_block_for(w, true));
    for (size_t e = 0; e < envs.size(); ++e) {
        for (const std::string &name : names) unsetenv(name.c_str());
        for (const auto &kv : envs[e]) setenv(kv.first.c_str(), kv.second.c_str(), 1);
        const fbplan::FbSwitches sw = fbplan::FbSwitches::read();
        std::printf("switches %zu %d %d %d %d %d %d %d %d %d %d %d %d\n", e, sw.ring, sw.ring_min_nd, sw.ring_split, sw.deep, sw.deep_min_nd,
                    sw.band_min_nd, sw.groups_set, sw.groups, sw.slots_x16, sw.split, sw.bwd_first, sw.decode_ring);
        for (size_t p = 0; p < pairs.size(); ++p) {
            fbplan::FbPlan plan;
            const int rc = fbplan::fb_plan_pair(&pairs[p].left.g, &pairs[p].right.g, pairs[p].band.n ? &pairs[p].band : nullptr, sw, &plan);
            std::printf("plan %zu %s %d", e, pairs[p].name.c_str(), rc);
            if (rc == PAGAN_OK) {
                std::printf(" %d |", plan.schedule());
                print_all(plan.info);
                std::printf(" | %d %d %d %zu %d %zu %zu %d %d |", plan.groups, plan.block, plan.nsplit, plan.init_at.size(), plan.init_dmin,
                            plan.seg_B.size(), plan.dfar.size(), plan.decode_route, plan.decode_block);
                for (const auto &c : caps) std::printf(" %d %d", plan.groups_within(c.first), plan.groups_within(c.second));
                std::printf(" |"); print_all(plan.init_at);
                std::printf(" |"); print_all(plan.seg_start);
                std::printf(" |"); print_all(plan.seg_B);
                std::printf(" |");
                for (size_t d = 0, z; d < plan.dfar.size(); d = z) {
                    for (z = d + 1; z < plan.dfar.size() && plan.dfar[z] == plan.dfar[d];) ++z;
                    std::printf(" %d:%zu", plan.dfar[d], z - d);
                }
            }
            std::printf("\n");
        }
    }
    return 0;
}
