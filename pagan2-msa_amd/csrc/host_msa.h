// host_msa.h -- the tree walk's state and the few internals its parts share: host_tree.cpp (the walk), host_rows.cpp (what
// reads the finished alignment), host_capi.cpp (the C wrappers that take no pagan_msa).  Private to csrc/.
#pragma once
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/pagan_host.h"
#include "host_anchors.h"
#include "host_graph.h"
#include "host_job.h"
#include "host_model.h"

struct pagan_hgraph { pagan::SeqGraph g; };

namespace pagan {

inline double now_s() {
    return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

template <class F> void parallel_for(int n, int threads, F f) {
    if (threads <= 1 || n <= 1) { for (int i = 0; i < n; ++i) f(i); return; }
    std::atomic<int> next(0);
    std::vector<std::thread> pool;
    const int t = std::min(threads, n);
    for (int k = 0; k < t; ++k) pool.emplace_back([&] { for (int i; (i = next.fetch_add(1)) < n;) f(i); });
    for (auto &th : pool) th.join();
}

// The walk's environment switches, read once per entry point on the calling thread and handed down (never cached across
// calls: a process may change them between walks).
struct HostSwitches {
    int host_threads_cap;        // PAGAN_HOST_THREADS: at most this many threads prepare the leaves (0: not set)
    enum { PARENTS_AUTO, PARENTS_HOST, PARENTS_DEVICE } parents;     // PAGAN_PARENTS=host / device forces either builder
    bool verbose;                // PAGAN_DP_VERBOSE
    static HostSwitches read() {
        const char *t = std::getenv("PAGAN_HOST_THREADS"), *p = std::getenv("PAGAN_PARENTS");
        return HostSwitches{t ? std::max(1, std::atoi(t)) : 0,
                            p && std::strcmp(p, "host") == 0 ? PARENTS_HOST : p && std::strcmp(p, "device") == 0 ? PARENTS_DEVICE : PARENTS_AUTO,
                            std::getenv("PAGAN_DP_VERBOSE") != nullptr};
    }
};

struct TreeNode {
    int left = -1, right = -1, parent = -1;
    double dist = 0;             // distance to parent after correction
    std::string name;
    int leaf_index = -1;         // input sequence index for leaves
};

struct NodeWork {                // everything one internal node's alignment consumed / produced
    int node = -1, level = 0;
    std::shared_ptr<EvolModel> model;
    NodeJob job;                 // job.res is held: aligned here, or imported from the rank that aligned it
    std::vector<TunnelBlock> blocks;     // empty tunnel blocks, ascending by size (anchor_mode 1; --force-gap takes the last)
    int n_hits = 0, n_forced = 0;
    int imp_l = 0, imp_r = 0;    // sites of the children of a node whose result was imported (pagan_msa_import_result)
    pagan_model pm;
    bool has_job = false;        // job's graphs and band and pm are valid: this process prepared and aligned the node
    int  device = -1;            // device the alignment ran on (-1: another rank)
    bool parent_pending = false; // imported: the result is stored, the parent graph is built when somebody needs it (ensure_graph)
    // the forward/backward pass of the node (full_probability / sample_path), on the band the node finally used
    bool has_fb = false;
    double log_fwd = 0, log_bwd = 0, fb_sweep_ms = 0, fb_post_ms = 0;
    std::vector<double> support;         // [res.n_cols] posterior of every column's own cell, -1 at skip columns
    bool has_marg = false;               // full_probability == 2: the site marginals (pagan_fb_site_marginals' eight arrays)
    std::vector<double> mg_d[6];         // pX, pM_left, best_p_left [Lx]; pY, pM_right, best_p_right [Ly]
    std::vector<int32_t> mg_i[2];        // best_j [Lx], best_i [Ly]
    // posterior decoding (pagan_msa_set_decoder): the node's result is the replay of its maximum expected accuracy path
    bool has_dec = false;
    double dec_objective = 0, dec_steps = 0, dec_ms = 0;   // dec_ms: the sub-batch's fill + trace, booked at its first node
    // expected counts (pagan_msa_set_counts): pagan_fb_expected_counts' trans[12] and, for DNA, emit[S * S]
    bool has_counts = false;
    double trans[12] = {0};
    std::vector<double> emit;
};

} // namespace pagan

struct pagan_msa {
    pagan_msa_opts opts;
    std::vector<std::string> names, seqs;
    std::vector<pagan::TreeNode> tree;   // as parsed
    int root = -1;
    std::vector<int> id_of_tree;         // tree index -> public node id
    std::vector<int> tree_of_id;         // public id -> tree index
    std::vector<std::unique_ptr<pagan_hgraph>> graph;    // by public node id
    std::vector<pagan::NodeWork> work;   // by internal order k (public id = n_leaves + k)
    pagan::ModelFactory mf;
    pagan_msa_timing tm;
    bool aligned = false;
    int n_leaves = 0;
    std::vector<std::string> rows;
    // walk state (pagan_msa_ready / align_nodes / import_result)
    std::vector<char> done;              // by public node id
    int remaining = 0, rounds = 0;
    std::map<double, std::shared_ptr<pagan::EvolModel>> model_cache;    // one table per distinct distance
    std::mutex mu;                       // model cache, timing sums
    std::vector<int32_t> state_table;    // parent state of a matched column: parsimony table, or with --mostcommon the
                                         // most-common table where it is defined (basic_alignment.cpp:146-149)
    pagan_batch_fn backend = nullptr;    // test seam (pagan_msa_set_batch_backend); null = pagan_dp_align_batch
    void *backend_user = nullptr;
    int sample_on_device = 0;            // pagan_msa_set_sampler: sample_path's paths come from pg_fb_sample (1) or the host's walk (0)
    int decode_on = 0;                   // pagan_msa_set_decoder: the nodes' results are their posteriors' maximum expected accuracy paths
    double decode_gap = 0.5;             // ... with this gap weight
    bool indel_set = false;              // pagan_msa_set_indel_model replaced a rate of the data type's defaults
    int counts_on = 0;                   // pagan_msa_set_counts: every forward/backward pass also leaves the node's expected counts
    std::atomic<int> parents_built{0};   // parent graphs this process has built (pagan_msa_parents_built)
    std::atomic<int> lazy_err{0};        // first error of a deferred parent build (an imported result that does not fit the child graphs)
    bool rows_built = false;             // m->rows are valid (pagan_msa_finish builds them at once, pagan_msa_finish_lazy on first use)
    std::mutex lazy_mu;                  // deferred builds started from the accessors
    // pagan_msa_ancestral's result: row k is internal node n + k's state of largest posterior per column, and that posterior
    bool anc_done = false;
    std::vector<uint8_t> anc_best;
    std::vector<float> anc_best_p;
};

namespace pagan {

int host_threads_of(const pagan_msa *m);                  // host_tree.cpp
int ensure_graph(pagan_msa *m, int id);                   // host_tree.cpp
int ensure_rows(pagan_msa *m, const HostSwitches &sw);    // host_rows.cpp

} // namespace pagan
