// host_tree.cpp -- the guide-tree walk of include/pagan_host.h: the tree, the nodes' jobs, their forward/backward pass, the two
// schedulers, results across processes, the per-node accessors.  (host_rows.cpp: what reads the finished alignment;
// host_capi.cpp: the entries that take no pagan_msa; host_msa.h: the state they share.)
//
// Counterpart of Node::start_openmp_alignment / align_sequences_this_node
// (src/main/node.cpp:52-285): nodes whose two children carry a sequence graph are "ready"
// (build_queues, node.cpp:273-285); each round aligns every ready node -- here as ONE batched
// GPU launch per device instead of one OpenMP task per node -- then builds the parents' graphs
// and promotes the nodes that became ready.  Rounds are the guide tree's levels.  Devices are
// fed by one host thread each from a shared list of ready nodes; there is no exchange step
// between devices (parents are built on the host), hence no collective.
#include <hip/hip_runtime.h>

#include <condition_variable>
#include <cmath>
#include <cstdio>
#include <sched.h>

#include "host_msa.h"

using namespace pagan;

namespace {

// Node::set_distance_to_parent, src/main/node.h:122-159 (defaults: no --scale-branches,
// no --real-branches, --truncate-branches 0.2 always active).
double corrected_branch(double d, float truncate) {
    if (d <= 0) d = 0.001;
    if (truncate > 0 && d > truncate) d = truncate;
    return d;
}

// Minimal Newick reader: rooted, strictly binary, names on leaves, optional lengths.
struct Newick {
    const char *p;
    std::vector<TreeNode> *nodes;
    bool ok = true;
    void ws() { while (*p == ' ' || *p == '\n' || *p == '\t' || *p == '\r') ++p; }
    int parse() {
        ws();
        int id;
        if (*p == '(') {
            ++p;
            const int l = parse();
            ws();
            if (*p != ',') { ok = false; return -1; }
            ++p;
            const int r = parse();
            ws();
            if (*p != ')') { ok = false; return -1; }     // multifurcations are not resolved here
            ++p;
            if (!ok) return -1;
            id = (int)nodes->size();
            nodes->push_back(TreeNode());
            (*nodes)[id].left = l; (*nodes)[id].right = r;
            (*nodes)[l].parent = id; (*nodes)[r].parent = id;
            ws();
            while (*p && *p != ':' && *p != ',' && *p != ')' && *p != ';') ++p;   // internal label ignored
        } else {
            const char *s = p;
            while (*p && *p != ':' && *p != ',' && *p != ')' && *p != ';' && *p != '(') ++p;
            if (p == s) { ok = false; return -1; }
            id = (int)nodes->size();
            nodes->push_back(TreeNode());
            (*nodes)[id].name.assign(s, p - s);
            while (!(*nodes)[id].name.empty() && (*nodes)[id].name.back() == ' ') (*nodes)[id].name.pop_back();
        }
        ws();
        if (*p == ':') {
            ++p;
            char *end = nullptr;
            (*nodes)[id].dist = std::strtod(p, &end);
            if (end == p) { ok = false; return -1; }
            p = end;
        }
        return id;
    }
};

int device_budget(const pagan_msa *m, int dev, int64_t *bytes) {
    const pagan_msa_opts &o = m->opts;
    if (o.device_mem_budget > 0) { *bytes = o.device_mem_budget; return PAGAN_OK; }
    if (m->backend) { *bytes = (int64_t)1 << 40; return PAGAN_OK; }
    if (hipSetDevice(dev) != hipSuccess) return PAGAN_E_NODEVICE;
    size_t fr = 0, tot = 0;
    if (hipMemGetInfo(&fr, &tot) != hipSuccess) return PAGAN_E_NODEVICE;
    *bytes = (int64_t)(0.8 * (double)(fr + (size_t)pagan_dp_cached_device_bytes(dev)));   // idle arenas are reused or dropped
    return PAGAN_OK;
}

// Aligns the nodes `ks` (indices into m->work) on device `dev`, splitting into sub-batches that
// fit the memory budget.
int align_on_device(pagan_msa *m, const std::vector<int> &ks, int dev, double *fill_ms, double *trace_ms) {
    int64_t budget = 0;
    int rc = device_budget(m, dev, &budget);
    if (rc != PAGAN_OK) return rc;
    pagan_opts po;
    po.flags = m->opts.dp_flags; po.device = dev;
    size_t at = 0;
    while (at < ks.size()) {
        std::vector<pagan_job> jobs;
        std::vector<int> which;
        int64_t used = 0;
        while (at < ks.size()) {
            NodeWork &w = m->work[ks[at]];
            const int64_t need = pagan_dp_predict_bytes(w.job.gl.n_sites, w.job.gr.n_sites, w.job.band());
            if (need < 0) return (int)need;
            if (need > budget) return PAGAN_E_MEMCAP;
            if (!jobs.empty() && used + need > budget) break;
            used += need;
            jobs.push_back(w.job.job(&w.pm)); which.push_back(ks[at]); ++at;
        }
        std::vector<pagan_result> res(jobs.size());
        rc = call_aligner(m->backend, m->backend_user, (int32_t)jobs.size(), jobs.data(), &po, res.data());
        if (rc != PAGAN_OK) return rc;            // nothing in res[] is valid then (the library released it): adopted after PAGAN_OK only
        for (size_t k = 0; k < jobs.size(); ++k) m->work[which[k]].job.res.adopt(res[k]);
        if (!res.empty()) { *fill_ms += res[0].fill_ms; *trace_ms += res[0].trace_ms; }
    }
    return PAGAN_OK;
}

// The compute_full_score pass of the nodes `ks` on device `dev` (viterbi_alignment.cpp:329-371), behind their Viterbi batch:
// pagan_fb_run_batch in sub-batches that fit the memory budget by pagan_fb_predict_bytes, the model's probability-space view
// at the node's distance, the band the node finally used.  Per node: the totals, the support of its path's columns (one
// gather), with full_probability == 2 the site marginals (one launch per pass and sub-batch).  The handles are destroyed before
// this returns: before the parents are built.
// sample_path: there was no Viterbi batch; the node's result is a path sampled from its forward matrix on the host
// (pagan_fb_sample_path downloads the matrix: 24 B a cell) with the numbers pagan_sample_uniforms gives for (sample_seed, public
// node id) -- no state shared between nodes, so neither batching nor the device that took a node changes its path.  A banded
// node whose full probability is 0 is handed back in `retry` (run again without the band, as an unreachable Viterbi corner is).
// With the sampler on the device (pagan_msa_set_sampler) the sub-batch's paths are drawn by one pagan_fb_sample_paths_batch
// instead -- the same numbers, the same paths -- and a node's result is the replay of its path 0: 12 B a path step come to the
// host, not the matrix.
// Posterior decoding (pagan_msa_set_decoder): no Viterbi batch either; the sub-batches are cut by pagan_fb_predict_bytes +
// pagan_fb_decode_predict_bytes, each goes through one pagan_fb_decode_batch behind its sweeps, and a node's result is the
// replay of its decoded path (score = log full probability, support along that path, the same retry without the band).
// In four steps: fb_cut, fb_sweeps, fb_paths + fb_node, fb_readers.

// what the pass does beside the sweeps: where a node's path comes from (path: from this pass at all), which readers run
struct FbMode {
    bool decode, path, device_sampler, marg, counts;
    explicit FbMode(const pagan_msa *m)
        : decode(m->decode_on != 0), path(m->opts.sample_path != 0 || decode), device_sampler(path && !decode && m->sample_on_device != 0),
          marg(m->opts.full_probability == 2), counts(m->counts_on != 0) {}
};

// A sub-batch: its nodes (indices into m->work) and their handles, destroyed with it on every exit
struct FbSub {
    std::vector<int> which;
    std::vector<pagan_fb *> fbs;
    std::vector<pagan_fb_samples *> smp;
    std::vector<pagan_fb_decoded *> dec;
    std::vector<char> again;                 // banded, full probability 0: goes to `retry`
    double smp_ms = 0, dec_ms = 0;
    explicit FbSub(const std::vector<int> &nodes)
        : which(nodes), fbs(nodes.size(), nullptr), smp(nodes.size(), nullptr), dec(nodes.size(), nullptr), again(nodes.size(), 0) {}
    FbSub(const FbSub &) = delete;
    ~FbSub() {                               // the path handles before the passes they are paths of
        for (pagan_fb_decoded *d : dec) pagan_fb_decoded_destroy(d);
        for (pagan_fb_samples *s : smp) pagan_fb_samples_destroy(s);
        for (pagan_fb *fb : fbs) pagan_fb_destroy(fb);
    }
};

// the nodes of ks from *at on that fit the budget together (one at least), by the sum of the mode's predictors
int fb_cut(const pagan_msa *m, const FbMode &md, const std::vector<int> &ks, size_t *at, int64_t budget, std::vector<int> *which) {
    int64_t used = 0;
    for (; *at < ks.size(); ++*at) {
        const NodeJob &j = m->work[ks[*at]].job;
        const pagan_band *band = j.band();
        int64_t need = pagan_fb_predict_bytes_states(j.gl.n_sites, j.gr.n_sites, band, m->mf.S);
        if (need < 0) return (int)need;
        if (md.decode) {
            const int64_t more = pagan_fb_decode_predict_bytes(j.gl.n_sites, j.gr.n_sites, band);
            if (more < 0) return (int)more;
            need += more;
        } else if (md.device_sampler) need += pagan_fb_sample_predict_bytes(j.gl.n_sites, j.gr.n_sites, 1, 0);    // (the path's trace)
        if (md.counts) need += pagan_fb_counts_predict_bytes(j.gl.n_sites, j.gr.n_sites, m->mf.S);
        if (need > budget) return PAGAN_E_MEMCAP;
        if (!which->empty() && used + need > budget) break;
        used += need;
        which->push_back(ks[*at]);
    }
    return PAGAN_OK;
}

int fb_sweeps(pagan_msa *m, FbSub &sb, int dev) {
    const int n = (int)sb.which.size();
    pagan_opts po;
    po.flags = 0; po.device = dev;
    std::vector<pagan_model_prob> mp(n);
    std::vector<const pagan_graph *> gl(n), gr(n);
    std::vector<const pagan_model_prob *> mpp(n);
    std::vector<const pagan_band *> bd(n);
    for (int q = 0; q < n; ++q) {
        NodeWork &w = m->work[sb.which[q]];
        mp[q] = w.model->prob_view();
        gl[q] = &w.job.gl; gr[q] = &w.job.gr; mpp[q] = &mp[q]; bd[q] = w.job.band();
    }
    return pagan_fb_run_batch(n, gl.data(), gr.data(), mpp.data(), bd.data(), &po, sb.fbs.data());
}

// the sub-batch's paths where the device makes them: one call of the decoder or of the sampler, and its time
int fb_paths(pagan_msa *m, const FbMode &md, FbSub &sb) {
    const int n = (int)sb.which.size();
    int rc = PAGAN_OK;
    if (md.decode) {
        double dms[2] = {0, 0};
        rc = pagan_fb_decode_batch(n, sb.fbs.data(), m->decode_gap, 0, sb.dec.data());
        if (rc == PAGAN_OK) rc = pagan_fb_decoded_ms(sb.dec[0], dms);
        sb.dec_ms = dms[0] + dms[1];
    } else if (md.device_sampler) {
        std::vector<int32_t> ids(n);
        for (int q = 0; q < n; ++q) ids[q] = m->work[sb.which[q]].node;
        rc = pagan_fb_sample_paths_batch(n, sb.fbs.data(), m->opts.sample_seed, ids.data(), 1, 0, sb.smp.data());
        if (rc == PAGAN_OK) rc = pagan_fb_samples_ms(sb.smp[0], &sb.smp_ms);
    }
    return rc;
}

// node q: the totals; where this pass gives the path, the result from its source (the decoder, the device's sampler, the host's);
// the support of the path's columns
int fb_node(pagan_msa *m, const FbMode &md, FbSub &sb, int q) {
    NodeWork &w = m->work[sb.which[q]];
    double ms[2] = {0, 0};
    int r = pagan_fb_totals(sb.fbs[q], &w.log_fwd, &w.log_bwd, nullptr);
    if (r == PAGAN_OK) r = pagan_fb_kernel_ms(sb.fbs[q], ms);
    w.fb_sweep_ms = ms[0] + ms[1]; w.fb_post_ms = 0;
    w.has_marg = false; w.support.clear(); w.has_dec = false;
    if (r == PAGAN_OK && md.path) {
        w.job.res.reset();                                                   // (a banded first attempt's, when this is the retry)
        if (!(w.log_fwd > -HUGE_VAL) && w.job.banded) { sb.again[q] = 1; return PAGAN_OK; }
        pagan_result raw;
        if (sb.dec[q]) {
            int32_t steps = 0;
            r = pagan_fb_decoded_summary(sb.dec[q], nullptr, &w.dec_objective, &steps, nullptr, nullptr);
            if (r == PAGAN_OK) r = pagan_fb_decoded_result(sb.dec[q], &raw);
            w.dec_steps = steps; w.dec_ms = q == 0 ? sb.dec_ms : 0.0;
            w.has_dec = r == PAGAN_OK;
        } else if (sb.smp[q]) {
            r = pagan_fb_samples_result(sb.smp[q], 0, &raw);
        } else {
            const int n_u = w.job.gl.n_sites + w.job.gr.n_sites - 1;         // Lx + Ly + 1
            std::vector<double> u((size_t)n_u);
            r = pagan_sample_uniforms(m->opts.sample_seed, w.node, n_u, u.data());
            if (r == PAGAN_OK) r = pagan_fb_sample_path(sb.fbs[q], u.data(), n_u, &raw, nullptr, nullptr);
        }
        if (r == PAGAN_OK) w.job.res.adopt(raw);
    }
    const pagan_result &res = w.job.res.get();
    if (r == PAGAN_OK && res.status == PAGAN_DP_REACHED) {
        w.support.assign((size_t)res.n_cols, 0.0);
        r = pagan_fb_path_support(sb.fbs[q], res.cols, res.n_cols, w.support.data());
    }
    return r;
}

// The readers over the whole sub-batch, one launch each (not for a node that goes to `retry`), while rc is PAGAN_OK; then what the
// sub-batch leaves at its nodes either way.  Times: a node's own gather and marginal passes; the sampler's at the first node, the
// counts' at the first node that stays.
int fb_readers(pagan_msa *m, const FbMode &md, const FbSub &sb, int rc, std::vector<int> *retry) {
    const int n = (int)sb.which.size();
    if (rc == PAGAN_OK && md.marg) {
        std::vector<double *> pd[6];
        std::vector<int32_t *> pi[2];
        for (int q = 0; q < n; ++q) {
            NodeWork &w = m->work[sb.which[q]];
            const size_t Lx = (size_t)w.job.gl.n_sites - 1, Ly = (size_t)w.job.gr.n_sites - 1;
            for (int a = 0; a < 6; ++a) { w.mg_d[a].assign(a < 3 ? Lx : Ly, 0.0); pd[a].push_back(sb.again[q] ? nullptr : w.mg_d[a].data()); }
            for (int a = 0; a < 2; ++a) { w.mg_i[a].assign(a < 1 ? Lx : Ly, 0); pi[a].push_back(sb.again[q] ? nullptr : w.mg_i[a].data()); }
            w.has_marg = !sb.again[q];
        }
        rc = pagan_fb_site_marginals_batch(n, sb.fbs.data(), pd[0].data(), pd[1].data(), pi[0].data(), pd[2].data(),
                                           pd[3].data(), pd[4].data(), pi[1].data(), pd[5].data());
    }
    double cnt_ms = 0;
    for (int q = 0; q < n; ++q) m->work[sb.which[q]].has_counts = false;
    if (rc == PAGAN_OK && md.counts) {
        // before the matrices are released; the emission table for DNA only
        const bool em = m->mf.type == kDna;
        std::vector<pagan_fb *> cf;
        std::vector<double *> ct, ce;
        for (int q = 0; q < n; ++q) {
            if (sb.again[q]) continue;
            NodeWork &w = m->work[sb.which[q]];
            w.emit.assign(em ? (size_t)m->mf.S * m->mf.S : 0, 0.0);
            cf.push_back(sb.fbs[q]); ct.push_back(w.trans); ce.push_back(em ? w.emit.data() : nullptr);
        }
        if (!cf.empty()) {
            rc = pagan_fb_expected_counts_batch((int32_t)cf.size(), cf.data(), ct.data(), ce.data());
            if (rc == PAGAN_OK) rc = pagan_fb_counts_ms(cf[0], &cnt_ms);
        }
        for (int q = 0; q < n; ++q) m->work[sb.which[q]].has_counts = rc == PAGAN_OK && !sb.again[q];
    }
    bool first_kept = true;
    for (int q = 0; q < n; ++q) {
        NodeWork &w = m->work[sb.which[q]];
        double ms[3] = {0, 0, 0};
        if (rc == PAGAN_OK && pagan_fb_post_ms(sb.fbs[q], ms) == PAGAN_OK) w.fb_post_ms = ms[0] + ms[1] + ms[2] + (q == 0 ? sb.smp_ms : 0.0);
        if (rc == PAGAN_OK && !sb.again[q] && first_kept) { w.fb_post_ms += cnt_ms; first_kept = false; }
        w.has_fb = rc == PAGAN_OK && !sb.again[q];
        w.has_dec = w.has_dec && w.has_fb;
        if (sb.again[q]) retry->push_back(sb.which[q]);
    }
    return rc;
}

int fb_on_device(pagan_msa *m, const std::vector<int> &ks, int dev, int threads, std::vector<int> *retry) {
    int64_t budget = 0;
    int rc = device_budget(m, dev, &budget);
    const FbMode md(m);
    for (size_t at = 0; rc == PAGAN_OK && at < ks.size();) {
        std::vector<int> which;
        rc = fb_cut(m, md, ks, &at, budget, &which);
        if (rc != PAGAN_OK) break;
        FbSub sb(which);
        rc = fb_sweeps(m, sb, dev);
        if (rc == PAGAN_OK) rc = fb_paths(m, md, sb);
        if (rc != PAGAN_OK) break;
        std::vector<int> rcs(which.size(), PAGAN_OK);
        parallel_for((int)which.size(), threads, [&](int q) { rcs[q] = fb_node(m, md, sb, q); });
        for (size_t q = 0; q < rcs.size() && rc == PAGAN_OK; ++q) rc = rcs[q];
        rc = fb_readers(m, md, sb, rc, retry);
    }
    return rc;
}

} // namespace

extern "C" {

void pagan_msa_default_opts(pagan_msa_opts *o) {
    std::memset(o, 0, sizeof(*o));
    o->use_anchors = 1; o->anchors_offset = 15; o->prefix_hit_length = 30; o->hit_trim = 5;
    o->truncate_branches = 0.2f;
    o->force_gap_threshold = 40000; o->overlap_total = 50; o->overlap_partly = 400;      // settings.cpp:180-189
}

int pagan_msa_create(int32_t n_seqs, const char *const *names, const char *const *seqs, const char *newick,
                     const pagan_msa_opts *opts, pagan_msa **out) {
    if (n_seqs < 2 || !names || !seqs || !newick || !out) return PAGAN_E_ARG;
    std::unique_ptr<pagan_msa> m(new pagan_msa());
    if (opts) m->opts = *opts; else pagan_msa_default_opts(&m->opts);
    m->n_leaves = n_seqs;
    std::map<std::string, int> by_name;
    m->seqs.resize(n_seqs);
    for (int k = 0; k < n_seqs; ++k) {
        if (!names[k] || !seqs[k]) return PAGAN_E_ARG;
        m->names.push_back(names[k]);
        by_name[m->names.back()] = k;
    }
    // per-leaf work (cleaning the residues here, the leaf graphs below) runs on a few threads: 32 x 100 kb
    // leaves are 0.2 s of the tree's 1.3 s otherwise
    const HostSwitches sw = HostSwitches::read();
    int nt = std::min(8, host_threads_of(m.get()));                 // allocation-heavy: oversubscribed, it is slower than serial
    if (sw.host_threads_cap > 0) nt = std::min(nt, sw.host_threads_cap);
    auto over_leaves = [&](auto f) { parallel_for(n_seqs, nt, f); };
    // fasta_reader.cpp:138-160: upper case, no gaps, no line ends
    over_leaves([&](int k) {
        std::string s;
        s.reserve(std::strlen(seqs[k]));
        for (const char *p = seqs[k]; *p; ++p) {
            const char c = (char)std::toupper((unsigned char)*p);
            if (c != '-' && c != '\r' && c != '\n') s.push_back(c);
        }
        m->seqs[k].swap(s);
    });
    // data_type 3: --codons on DNA input (input_output_parser.cpp:517, sequence.cpp:135-136)
    int type = m->opts.data_type == 1 ? kDna : m->opts.data_type == 2 ? kProtein : m->opts.data_type == 3 ? kCodon : ModelFactory::guess_type(m->seqs);
    // Fasta_reader::check_alphabet, fasta_reader.cpp:1180-1297: DNA U->T; protein U->X; what is outside the
    // full alphabet is dropped
    {
        char keep[256];                                            // 0: dropped, else the character it becomes
        std::memset(keep, 0, sizeof(keep));
        for (const char *p = type != kProtein ? ModelFactory::dna_full_alphabet() : ModelFactory::protein_alphabet(); *p; ++p)
            keep[(unsigned char)*p] = *p;
        if (type != kProtein) keep[(unsigned char)'U'] = 'T'; else keep[(unsigned char)'U'] = keep[(unsigned char)'X'] = 'X';
        over_leaves([&](int k) {
            std::string &s = m->seqs[k];
            size_t w = 0;
            for (size_t r = 0; r < s.size(); ++r) { const char c = keep[(unsigned char)s[r]]; if (c) s[w++] = c; }
            s.resize(w);
        });
    }
    Newick nw{newick, &m->tree};
    m->root = nw.parse();
    if (!nw.ok || m->root < 0) return PAGAN_E_TREE;
    nw.ws();
    if (*nw.p == ';') ++nw.p;
    int n_leaf_nodes = 0;
    for (auto &t : m->tree) {
        if (t.left < 0) {
            auto it = by_name.find(t.name);
            if (it == by_name.end() || it->second < 0) return PAGAN_E_TREE;
            t.leaf_index = it->second; it->second = -1; ++n_leaf_nodes;
        }
        t.dist = corrected_branch(t.dist, m->opts.truncate_branches);
    }
    if (n_leaf_nodes != n_seqs || (int)m->tree.size() != 2 * n_seqs - 1) return PAGAN_E_TREE;
    // public ids: leaves by input order, internal nodes in parse order -- the parser closes a
    // node after both children, i.e. post-order left->right->self, the reference's alignment
    // order and #k# naming (src/main/node.h:479-495,928-938).
    m->id_of_tree.assign(m->tree.size(), -1);
    m->tree_of_id.assign(m->tree.size(), -1);
    int next_internal = n_seqs;
    for (size_t t = 0; t < m->tree.size(); ++t) {
        const int id = m->tree[t].left < 0 ? m->tree[t].leaf_index : next_internal++;
        m->id_of_tree[t] = id; m->tree_of_id[id] = (int)t;
    }
    m->graph.resize(m->tree.size());
    if (type == kDna) {
        float bf[4];
        ModelFactory::base_frequencies(m->seqs, bf);
        m->mf.init_dna(bf);
    } else if (type == kCodon) {
        m->mf.init_codon();
    } else {
        m->mf.init_protein();
    }
    m->state_table = m->mf.parsimony;
    if (m->opts.mostcommon)      // Evol_model::mostcommon_state: defined over mc_dim x mc_dim states (20 x 20 residues for protein)
        for (int i = 0; i < m->mf.mc_dim; ++i)
            for (int j = 0; j < m->mf.mc_dim; ++j) m->state_table[i + (size_t)j * m->mf.S] = m->mf.mostcommon[i + j * m->mf.mc_dim];
    over_leaves([&](int k) {
        m->graph[k].reset(new pagan_hgraph());
        if (type == kCodon) {
            std::string symbols;
            const std::vector<int32_t> states = ModelFactory::codon_states(m->seqs[k], &symbols);
            m->graph[k]->g = make_leaf_states(states, std::move(symbols), 3, 0);
        } else {
            m->graph[k]->g = make_leaf(m->seqs[k], m->mf.leaf_alphabet, m->opts.leaf_flags);
        }
    });
    m->work.resize(n_seqs - 1);
    m->done.assign(2 * n_seqs - 1, 0);
    for (int k = 0; k < n_seqs; ++k) m->done[k] = 1;
    m->remaining = n_seqs - 1;
    std::memset(&m->tm, 0, sizeof(m->tm));
    *out = m.release();
    return PAGAN_OK;
}

} // extern "C"

namespace {

// The threads the host-side phases use when the caller names none: what this process may actually run on -- the hardware's
// threads, cut down to the affinity mask and to the cgroup's CPU quota -- and at most 16 (round 5: a GPU box reports 256
// hardware threads to a process that owns a 16-core share; 256 threads per phase there made the rows 85-97 ms instead of 20,
// and every phase is memory- or allocation-bound well before 16).
int default_host_threads() {
    static const int cached = [] {
        long long t = (long long)std::thread::hardware_concurrency();
        if (t < 1) t = 1;
        cpu_set_t set;
        if (sched_getaffinity(0, sizeof set, &set) == 0 && CPU_COUNT(&set) > 0) t = std::min<long long>(t, CPU_COUNT(&set));
        long long quota = -1, period = 0;
        if (FILE *f = std::fopen("/sys/fs/cgroup/cpu.max", "r")) {                     // cgroup v2: "<quota|max> <period>"
            char q[32] = {0};
            if (std::fscanf(f, "%31s %lld", q, &period) == 2 && std::strcmp(q, "max") != 0) quota = std::atoll(q);
            std::fclose(f);
        } else {                                                                       // cgroup v1
            if (FILE *g = std::fopen("/sys/fs/cgroup/cpu/cpu.cfs_quota_us", "r")) { if (std::fscanf(g, "%lld", &quota) != 1) quota = -1; std::fclose(g); }
            if (FILE *g = std::fopen("/sys/fs/cgroup/cpu/cpu.cfs_period_us", "r")) { if (std::fscanf(g, "%lld", &period) != 1) period = 0; std::fclose(g); }
        }
        if (quota > 0 && period > 0) t = std::min(t, std::max(1ll, (quota + period - 1) / period));
        return (int)std::max(1ll, std::min(t, 16ll));
    }();
    return cached;
}

} // namespace

int pagan::host_threads_of(const pagan_msa *m) {
    const int threads = m->opts.host_threads > 0 ? m->opts.host_threads : default_host_threads();
    return threads < 1 ? 1 : threads;
}

namespace {

bool node_ready(const pagan_msa *m, int id) {
    if (m->done[id]) return false;
    const TreeNode &t = m->tree[m->tree_of_id[id]];
    return m->done[m->id_of_tree[t.left]] && m->done[m->id_of_tree[t.right]];
}

// What align_sequences_this_node does before the aligner is called (node.cpp:70-152): the model for
// dist = d_left + d_right (serialised in the reference too: omp critical, node.cpp:415-416), the
// child graphs' views, anchors -> tunnel.
void prepare_node(pagan_msa *m, int id, int round) {
    const int n = m->n_leaves;
    NodeWork &w = m->work[id - n];
    const TreeNode &t = m->tree[m->tree_of_id[id]];
    const double dist = m->tree[t.left].dist + m->tree[t.right].dist;         // node.cpp:70
    const bool pileup_rates = m->opts.pileup_rates != 0;
    {
        std::lock_guard<std::mutex> g(m->mu);
        auto it = m->model_cache.find(dist);
        if (it == m->model_cache.end())
            it = m->model_cache.emplace(dist, std::make_shared<EvolModel>(m->mf.alignment_model(dist, pileup_rates))).first;
        w.model = it->second;
    }
    w.node = id; w.level = round;
    {   // (rank mode: a child that another rank aligned gets its graph now -- and so does whatever is pending below it)
        int rc = ensure_graph(m, m->id_of_tree[t.left]);
        if (rc == PAGAN_OK) rc = ensure_graph(m, m->id_of_tree[t.right]);
        if (rc != PAGAN_OK) { int zero = 0; m->lazy_err.compare_exchange_strong(zero, rc); return; }
    }
    const SeqGraph &gl = m->graph[m->id_of_tree[t.left]]->g, &gr = m->graph[m->id_of_tree[t.right]]->g;
    NodeJob &j = w.job;
    j.gl = gl.view(); j.gr = gr.view(); w.pm = w.model->view();
    j.banded = false;
    if (m->opts.use_anchors) {
        AnchorSettings as;
        as.offset = m->opts.anchors_offset; as.prefix_hit_length = m->opts.prefix_hit_length; as.hit_trim = m->opts.hit_trim;
        // what the anchors are looked for in: the graph's string, or -- codon graphs -- its translation, one letter per site
        // (viterbi_alignment.cpp:54-60, 141-145)
        const bool codons = m->mf.type == kCodon;
        const std::string &alpha = codons ? m->mf.codon_names : m->mf.ancestral_alphabet;
        auto str = [&](const SeqGraph &g, bool with_gaps) {
            return codons ? ModelFactory::translate_codons(sequence_string(g, with_gaps, alpha)) : sequence_string(g, with_gaps, alpha);
        };
        if (m->opts.anchor_mode == 1) {
            // the reference's BLAST branch from the hit list onwards (viterbi_alignment.cpp:148-157): hits here are the
            // prefix anchors, sorted by length as find_long_substrings leaves them
            std::vector<Hit> hits;
            prefix_hits(str(gl, false), str(gr, false), as.prefix_hit_length, &hits);
            drop_bad_hits(&hits, (unsigned)m->opts.overlap_total, (unsigned)m->opts.overlap_partly);
            j.upper.clear(); j.lower.clear(); w.blocks.clear();
            hits_to_band_overlapping(hits, str(gl, true), str(gr, true), as.offset, &j.upper, &j.lower, &w.blocks);
            w.n_hits = (int)hits.size();
        } else {
            w.n_hits = define_tunnel(str(gl, false), str(gr, false), str(gl, true), str(gr, true), as, &j.upper, &j.lower);
        }
        j.set_band();
    }
    w.has_job = true;
}

// Node::get_ambiguous_states (node.cpp:1638-1659): the states below an ambiguous site, down to unambiguous ones.
void ambiguous_states(const pagan_msa *m, int id, int pos, std::vector<int> *out) {
    const SeqGraph &g = m->graph[id]->g;
    if (!g.ambiguous[pos]) { out->push_back(g.state[pos]); return; }
    const TreeNode &t = m->tree[m->tree_of_id[id]];
    if (t.left < 0) return;                                        // an ambiguous leaf site has nothing below it
    if (g.child_l[pos] >= 0) ambiguous_states(m, m->id_of_tree[t.left], g.child_l[pos], out);
    if (g.child_r[pos] >= 0) ambiguous_states(m, m->id_of_tree[t.right], g.child_r[pos], out);
}

// Node::set_ambiguous_state (node.cpp:1661-1690): pushes a resolved state down the ambiguous sites that carry it.
bool set_ambiguous_state(pagan_msa *m, int id, int pos, int state) {
    SeqGraph &g = m->graph[id]->g;
    if (!g.ambiguous[pos]) return g.state[pos] == state;
    const TreeNode &t = m->tree[m->tree_of_id[id]];
    if (t.left < 0) return false;
    bool cont = true;
    if (g.child_l[pos] >= 0 && set_ambiguous_state(m, m->id_of_tree[t.left], g.child_l[pos], state)) { g.state[pos] = state; cont = false; }
    if (g.child_r[pos] >= 0 && cont && set_ambiguous_state(m, m->id_of_tree[t.right], g.child_r[pos], state)) g.state[pos] = state;
    return false;
}

// Node::fix_ambiguous_states (node.cpp:1610-1636), --mostcommon only: a site whose two subtrees share exactly one state
// (and bring more than two states together) takes that state, and so do the ambiguous sites below it.
void fix_ambiguous_states(pagan_msa *m, int id) {
    const TreeNode &t = m->tree[m->tree_of_id[id]];
    const int lid = m->id_of_tree[t.left], rid = m->id_of_tree[t.right];
    const int n = m->graph[id]->g.n_sites();
    std::vector<int> ls, rs;
    for (int j = 1; j < n - 1; ++j) {
        const SeqGraph &g = m->graph[id]->g;
        ls.clear(); rs.clear();
        if (g.child_l[j] >= 0) ambiguous_states(m, lid, g.child_l[j], &ls);
        if (g.child_r[j] >= 0) ambiguous_states(m, rid, g.child_r[j], &rs);
        std::sort(ls.begin(), ls.end()); ls.erase(std::unique(ls.begin(), ls.end()), ls.end());       // std::set semantics
        std::sort(rs.begin(), rs.end()); rs.erase(std::unique(rs.begin(), rs.end()), rs.end());
        std::vector<int> both;
        std::set_intersection(ls.begin(), ls.end(), rs.begin(), rs.end(), std::back_inserter(both));
        if (both.size() == 1 && ls.size() + rs.size() > 2) set_ambiguous_state(m, id, j, both[0]);
    }
}

std::atomic<long long> parents_on_device{0};                     // (diagnostic: pagan_parents_device_calls)

// add_ancestral_sequence(va.get_simple_sequence()) (node.cpp:166): the parent graph from the path.
int build_parent(pagan_msa *m, int id, int unit_nodes, const HostSwitches &sw) {
    NodeWork &w = m->work[id - m->n_leaves];
    const pagan_result &res = w.job.res.get();
    if (!w.job.res.held() || res.status != PAGAN_DP_REACHED) return PAGAN_E_INTERNAL;
    BuildSettings bs;
    if (m->opts.keep_all_edges) bs.reads_mode();
    if (m->opts.dp_flags & PAGAN_OPT_NO_REDUCED_TERMINAL_PEN) bs.reduced_terminal = false;
    const TreeNode &t = m->tree[m->tree_of_id[id]];
    SeqGraph &gl = m->graph[m->id_of_tree[t.left]]->g, &gr = m->graph[m->id_of_tree[t.right]]->g;
    m->graph[id].reset(new pagan_hgraph());
    // The parent on the device the node was aligned on (dp_parent.hip; its copy there stays for the build one level up) when
    // the graphs are long enough for a dozen launches to beat one host thread's walk over the columns; PAGAN_PARENTS=host /
    // device forces either.  --mostcommon (round 5): the graph comes from the device all the same; fix_ambiguous_states then
    // rewrites states on the host -- of this node and of the ambiguous sites below it -- and the node's device copy, which the
    // build one level up reads its children's states from, takes the node's over (the graphs below have no device copy left).
    bool on_device = false;
    if (!m->backend && w.device >= 0) {
        const bool force_host = sw.parents == HostSwitches::PARENTS_HOST, force_dev = sw.parents == HostSwitches::PARENTS_DEVICE;
        // (a wide level's parents are built side by side on the host's threads, and as many uploads of leaf-sized children
        //  at once cost more than they save: measured on 32 x 100 kb, 16 nodes 17 ms on the device against 7 on 16 threads,
        //  one node 3 ms against 8-15; so the device takes the levels of at most four long nodes)
        if (!force_host && (force_dev || (res.n_cols >= 20000 && unit_nodes <= 4))) {
            SeqGraph g;
            if (make_parent_device(gl, gr, res, (float)m->tree[t.left].dist, (float)m->tree[t.right].dist, m->state_table.data(),
                                   m->mf.S, m->mf.char_as, bs, w.device, &g)) {
                m->graph[id]->g = std::move(g);
                on_device = true;
                parents_on_device.fetch_add(1);
            }
        }
    }
    if (!on_device)
        m->graph[id]->g = make_parent(gl, gr, res, (float)m->tree[t.left].dist, (float)m->tree[t.right].dist,
                                      m->state_table.data(), m->mf.S, m->mf.char_as, bs);
    // (grandchildren's device copies are no longer needed: their parents are built)
    gl.dev.reset(); gr.dev.reset();
    if (m->opts.mostcommon) {
        fix_ambiguous_states(m, id);
        if (on_device && !parent_update_states(m->graph[id]->g)) m->graph[id]->g.dev.reset();
    }
    w.parent_pending = false;
    m->parents_built.fetch_add(1);
    return PAGAN_OK;
}

// Sites of a node's graph -- of the graph itself, or, for an imported node whose parent graph has not been built yet, what
// it will have: one site per alignment column plus the start and the end site (create_ancestral_sequence,
// basic_alignment.cpp:61-179: skipped and later deleted columns stay as sites).
int sites_of(const pagan_msa *m, int id) {
    if (m->graph[id]) return m->graph[id]->g.n_sites();
    return m->work[id - m->n_leaves].job.res.get().n_cols + 2;
}

} // namespace

// The graph of node `id`, built now if it is an imported node's that nobody has needed so far -- together with whatever is
// pending below it, children first (iteratively: a caterpillar tree is as deep as it has leaves).  Rank mode (one process
// per GPU): a rank builds the parents of the nodes it aligns and of the imported nodes BELOW the nodes it claims; the rest
// only if it is asked for the rows (node.cpp:196-223, 273-345: a thread builds the ancestor of the node it aligned).
// Ready nodes have disjoint subtrees, so the units of a round may call this side by side.
int pagan::ensure_graph(pagan_msa *m, int id) {
    if (m->graph[id]) return PAGAN_OK;
    std::vector<int> stack{id};
    while (!stack.empty()) {
        const int cur = stack.back();
        if (m->graph[cur]) { stack.pop_back(); continue; }
        if (cur < m->n_leaves || !m->done[cur]) return PAGAN_E_INTERNAL;       // (a leaf always has its graph; a node that is not done has no path)
        const TreeNode &t = m->tree[m->tree_of_id[cur]];
        const int lid = m->id_of_tree[t.left], rid = m->id_of_tree[t.right];
        if (!m->graph[lid] || !m->graph[rid]) {
            if (!m->graph[lid]) stack.push_back(lid);
            if (!m->graph[rid]) stack.push_back(rid);
            continue;
        }
        NodeWork &w = m->work[cur - m->n_leaves];
        // what pagan_msa_import_result could not check without the child graphs: a column names a child site (1 .. n_sites - 2)
        // or none (-1) -- which of the two follows from its path state --, a used edge is an edge of the child
        const SeqGraph &gl = m->graph[lid]->g, &gr = m->graph[rid]->g;
        const pagan_result &r = w.job.res.get();
        bool good = w.job.res.held();
        for (int k = 0; good && k < r.n_cols; ++k) {
            const pagan_col &c = r.cols[k];
            const bool hl = c.path_state == PAGAN_MATCHED || c.path_state == PAGAN_XGAPPED || c.path_state == PAGAN_XSKIPPED;
            const bool hr = c.path_state == PAGAN_MATCHED || c.path_state == PAGAN_YGAPPED || c.path_state == PAGAN_YSKIPPED;
            if (hl ? (c.left < 1 || c.left > gl.n_sites() - 2) : c.left != -1) good = false;
            if (hr ? (c.right < 1 || c.right > gr.n_sites() - 2) : c.right != -1) good = false;
        }
        for (int k = 0; good && k < r.n_left_used; ++k) if (r.left_used[k] < 0 || r.left_used[k] >= gl.n_edges()) good = false;
        for (int k = 0; good && k < r.n_right_used; ++k) if (r.right_used[k] < 0 || r.right_used[k] >= gr.n_edges()) good = false;
        if (!good) return PAGAN_E_ARG;
        const double t0 = now_s();
        const int rc = build_parent(m, cur, 1 << 20, HostSwitches{0, HostSwitches::PARENTS_HOST, false});   // (imported: w.device is -1, the host builder)
        {
            std::lock_guard<std::mutex> g(m->mu);
            m->tm.build_s += now_s() - t0;
        }
        if (rc != PAGAN_OK) return rc;
        stack.pop_back();
    }
    return PAGAN_OK;
}

namespace {

// One unit of the work queue: the nodes `ids` (all ready) prepared, aligned on device `dev`, their parents
// built.  Runs on the calling thread (+ the host thread pool); several of these run side by side on
// different devices.  "anchored alignment failed: trying again" (viterbi_alignment.cpp:298-317): a node
// whose end corner is unreachable inside its tunnel is re-aligned over the full matrix.
int run_unit(pagan_msa *m, const std::vector<int> &ids, int dev, int round, int threads, const HostSwitches &sw) {
    const int n = m->n_leaves;
    double t0 = now_s();
    parallel_for((int)ids.size(), threads, [&](int r) { set_anchor_device(dev); prepare_node(m, ids[r], round); });
    if (const int e = m->lazy_err.load()) return e;
    const double t_prep = now_s() - t0;
    t0 = now_s();
    std::vector<int> ks(ids.size());
    std::vector<int64_t> cost(ids.size());
    if (m->opts.force_gap) {
        // the memory guard of align_sequences_this_node (node.cpp:81-152): while the alignment does not fit the budget,
        // the largest empty tunnel block is replaced by a gap-shaped tunnel; no block left -> the node fails
        int64_t budget = 0;
        int rc = device_budget(m, dev, &budget);
        if (rc != PAGAN_OK) return rc;
        for (int id : ids) {
            NodeWork &w = m->work[id - n];
            NodeJob &j = w.job;
            if (!j.banded) continue;
            while (pagan_dp_predict_bytes(j.gl.n_sites, j.gr.n_sites, &j.pb) > budget) {
                if (!force_gap(&j.upper, &j.lower, &w.blocks, m->opts.force_gap_threshold, m->opts.anchors_offset, m->opts.force_gap_wide != 0))
                    return PAGAN_E_MEMCAP;
                ++w.n_forced;
            }
        }
    }
    for (size_t r = 0; r < ids.size(); ++r) {
        NodeWork &w = m->work[ids[r] - n];
        cost[r] = pagan_dp_count_cells(w.job.gl.n_sites, w.job.gr.n_sites, w.job.band());
        if (cost[r] < 0) return (int)cost[r];
        w.device = dev;
    }
    std::vector<int> order(ids.size());
    for (size_t r = 0; r < ids.size(); ++r) order[r] = (int)r;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return cost[a] > cost[b]; });
    for (size_t r = 0; r < ids.size(); ++r) ks[r] = ids[order[r]] - n;
    double fill_ms = 0, trace_ms = 0;
    int rc = PAGAN_OK;
    const bool sample = m->opts.sample_path != 0 || m->decode_on != 0;       // (no Viterbi batch: the forward/backward pass gives the path)
    if (!sample) {
        rc = align_on_device(m, ks, dev, &fill_ms, &trace_ms);
        if (rc != PAGAN_OK) return rc;
        std::vector<int> retry;
        for (int k : ks) if (m->work[k].job.banded && m->work[k].job.res.get().status == PAGAN_DP_UNREACHABLE) retry.push_back(k);
        if (!retry.empty()) {
            for (int k : retry) { m->work[k].job.banded = false; m->work[k].job.res.reset(); }
            rc = align_on_device(m, retry, dev, &fill_ms, &trace_ms);
            if (rc != PAGAN_OK) return rc;
        }
    }
    if (sample || m->opts.full_probability) {
        // behind the retry: on the band the node finally used (--sample-path: in the Viterbi batch's place, VA:395-417)
        std::vector<int> retry, none;
        rc = fb_on_device(m, ks, dev, threads, &retry);
        if (rc != PAGAN_OK) return rc;
        if (!retry.empty()) {
            for (int k : retry) m->work[k].job.banded = false;
            rc = fb_on_device(m, retry, dev, threads, &none);
            if (rc != PAGAN_OK) return rc;
        }
        for (int k : ks) if (!m->work[k].job.res.held()) return PAGAN_E_INTERNAL;
    }
    const double t_dp = now_s() - t0;
    t0 = now_s();
    std::atomic<int> bad(0);
    parallel_for((int)ids.size(), threads, [&](int r) { if (build_parent(m, ids[r], (int)ids.size(), sw) != PAGAN_OK) bad = 1; });
    const double t_build = now_s() - t0;
    if (sw.verbose)
        std::fprintf(stderr, "pagan_msa: unit of %d node(s) on device %d: prepare (model, children, anchors, tunnel) %.1f ms, DP (plan, batch, kernels, fetch) %.1f ms, parents %.1f ms\n",
                     (int)ids.size(), dev, 1e3 * t_prep, 1e3 * t_dp, 1e3 * t_build);
    {
        std::lock_guard<std::mutex> g(m->mu);
        m->tm.anchors_s += t_prep; m->tm.dp_wall_s += t_dp; m->tm.build_s += t_build;
        m->tm.dp_fill_dev_s += fill_ms / 1e3; m->tm.dp_trace_dev_s += trace_ms / 1e3;
    }
    return bad ? PAGAN_E_INTERNAL : PAGAN_OK;     // unreachable end corner: caller may retry with use_anchors = 0
}

int64_t node_cost_estimate(const pagan_msa *m, int id) {
    const TreeNode &t = m->tree[m->tree_of_id[id]];
    const int64_t lx = sites_of(m, m->id_of_tree[t.left]), ly = sites_of(m, m->id_of_tree[t.right]);
    // before the anchors are known: a tunnel is ~ (2 * offset + a few) cells per row, a full matrix Lx * Ly
    return m->opts.use_anchors ? (lx + ly) * (int64_t)(2 * m->opts.anchors_offset + 16) : lx * ly;
}

// pagan_msa_set_indel_model: the rates give a positive non-gap probability 1 - 2 t, t = 1 - exp(-0.5 (ins + del) dist), at every
// internal node's distance (the float expressions of ModelFactory::alignment_model)
bool indel_model_fits(const pagan_msa *m) {
    if (!m->indel_set) return true;
    const bool pileup = m->opts.pileup_rates != 0;
    const float ins = pileup ? 0.25f : m->mf.ins_rate, del = pileup ? 0.25f : m->mf.del_rate;
    for (const TreeNode &t : m->tree) {
        if (t.left < 0 || t.right < 0) continue;
        const double dist = m->tree[t.left].dist + m->tree[t.right].dist;
        const double tt = 1.0 - std::exp(-0.5 * (ins + del) * dist);
        if (!(1.0 - 2 * tt > 0.0)) return false;
    }
    return true;
}

// What both schedulers refuse before anything runs, in this order
int walk_mode_check(const pagan_msa *m) {
    const bool pass = m->opts.full_probability || m->opts.sample_path || m->decode_on;
    if (m->decode_on && m->opts.sample_path) return PAGAN_E_ARG;        // (a node has one path: the decoded one or a sampled one)
    if (m->counts_on && !pass) return PAGAN_E_ARG;                      // (no pass to take the counts from)
    if (!indel_model_fits(m)) return PAGAN_E_ARG;
    if (m->backend && pass) return PAGAN_E_NODEVICE;                    // (the seam has no forward/backward pass: never skipped silently)
    return PAGAN_OK;
}

// the devices of the walk: opts' first_device / n_devices, or (n_devices <= 0) the caller's current device alone
int resolve_devices(const pagan_msa *m, int *first, int *n) {
    *n = m->opts.n_devices; *first = m->opts.first_device;
    if (*n <= 0) { *n = 1; if (!m->backend && hipGetDevice(first) != hipSuccess) return PAGAN_E_NODEVICE; }
    return PAGAN_OK;
}

// Internal node k where it has all of `what` (kAny: where it exists), else NULL: the per-node accessors' PAGAN_E_ARG
enum : unsigned { kAny = 0, kRes = 1, kJob = 2, kFb = 4, kMarg = 8, kDec = 16, kCounts = 32 };
const NodeWork *node_with(const pagan_msa *m, int32_t k, unsigned what) {
    if (!m || k < 0 || k >= m->n_leaves - 1) return nullptr;
    const NodeWork &w = m->work[k];
    const unsigned has = (w.job.res.held() ? kRes : 0) | (w.has_job ? kJob : 0) | (w.has_fb ? kFb : 0) | (w.has_marg ? kMarg : 0) |
                         (w.has_dec ? kDec : 0) | (w.has_counts ? kCounts : 0);
    return (what & ~has) ? nullptr : &w;
}

} // namespace

extern "C" {

int pagan_msa_ready(const pagan_msa *m, int32_t *ids, int32_t cap) {
    if (!m) return PAGAN_E_ARG;
    int cnt = 0;
    for (int id = m->n_leaves; id < 2 * m->n_leaves - 1; ++id)
        if (node_ready(m, id)) { if (ids && cnt < cap) ids[cnt] = id; ++cnt; }
    return cnt;
}

int pagan_msa_remaining(const pagan_msa *m) { return m ? m->remaining : PAGAN_E_ARG; }

int64_t pagan_msa_node_cost(const pagan_msa *m, int32_t id) {
    if (!m || id < m->n_leaves || id >= 2 * m->n_leaves - 1 || !node_ready(m, id)) return PAGAN_E_ARG;
    return node_cost_estimate(m, id);
}

// The in-process work queue (Node::start_threaded_alignment, node.cpp:196-223,289-345, with devices in the
// place of threads): whenever devices are idle and nodes are ready, the ready nodes are dealt over the idle
// devices (largest first, least-loaded device) and each device's share becomes one unit on its own feeder
// thread.  A parent becomes ready the moment its two children are done, whichever devices they ran on; a
// device that finishes early picks up what is ready without waiting for the others.
int pagan_msa_align_nodes(pagan_msa *m, int32_t n_ids, const int32_t *ids) {
    if (!m || m->aligned || n_ids < 0 || (n_ids > 0 && !ids)) return PAGAN_E_ARG;
    if (const int rc = walk_mode_check(m)) return rc;
    for (int k = 0; k < n_ids; ++k)
        if (ids[k] < m->n_leaves || ids[k] >= 2 * m->n_leaves - 1 || !node_ready(m, ids[k])) return PAGAN_E_ARG;
    if (n_ids == 0) return PAGAN_OK;
    const double t_start = now_s();
    int ndev = 0, first_dev = 0;
    if (const int rc = resolve_devices(m, &first_dev, &ndev)) return rc;
    const HostSwitches sw = HostSwitches::read();
    const int threads = host_threads_of(m);
    std::vector<int64_t> cost(n_ids);
    for (int k = 0; k < n_ids; ++k) cost[k] = node_cost_estimate(m, ids[k]);
    std::vector<int32_t> owner(n_ids);
    const int workers = std::min(ndev, (int)n_ids);
    pagan_assign_units(n_ids, cost.data(), workers, owner.data());
    std::vector<std::vector<int>> share(workers);
    for (int k = 0; k < n_ids; ++k) share[owner[k]].push_back(ids[k]);
    std::vector<int> rcs(workers, PAGAN_OK);
    const int round = m->rounds++;
    if (workers == 1) {
        rcs[0] = run_unit(m, share[0], first_dev, round, threads, sw);
    } else {
        std::vector<std::thread> feeders;
        const int per = std::max(1, threads / workers);
        for (int d = 0; d < workers; ++d)
            feeders.emplace_back([&, d] { rcs[d] = run_unit(m, share[d], first_dev + d, round, per, sw); });
        for (auto &th : feeders) th.join();
    }
    for (int rc : rcs) if (rc != PAGAN_OK) return rc;
    for (int k = 0; k < n_ids; ++k) { m->done[ids[k]] = 1; --m->remaining; }
    m->tm.total_s += now_s() - t_start;
    return PAGAN_OK;
}

int pagan_msa_finish(pagan_msa *m) {
    if (!m || m->aligned || m->remaining != 0) return PAGAN_E_ARG;
    m->aligned = true;
    return ensure_rows(m, HostSwitches::read());
}

// Rank mode: the walk is over, but this process may never be asked for the rows -- the graphs of the nodes other ranks
// aligned above its own are then never built here.  The first call that needs them (alignment length / rows / FASTA, a
// node's graph) builds what is pending.
int pagan_msa_finish_lazy(pagan_msa *m) {
    if (!m || m->aligned || m->remaining != 0) return PAGAN_E_ARG;
    m->aligned = true;
    return PAGAN_OK;
}

int pagan_msa_parents_built(const pagan_msa *m) { return m ? m->parents_built.load() : PAGAN_E_ARG; }

int pagan_msa_align(pagan_msa *m) {
    if (!m || m->aligned) return PAGAN_E_ARG;
    if (const int rc = walk_mode_check(m)) return rc;
    int ndev = 0, first_dev = 0;
    if (const int rc = resolve_devices(m, &first_dev, &ndev)) return rc;
    const HostSwitches sw = HostSwitches::read();
    const int threads = host_threads_of(m);
    if (ndev == 1) {
        // one device: every round takes all ready nodes as one batch (the guide tree's levels)
        std::vector<int32_t> ids(m->n_leaves);
        while (m->remaining > 0) {
            const int cnt = pagan_msa_ready(m, ids.data(), (int32_t)ids.size());
            if (cnt <= 0) return PAGAN_E_INTERNAL;
            const int rc = pagan_msa_align_nodes(m, cnt, ids.data());
            if (rc != PAGAN_OK) return rc;
        }
        return pagan_msa_finish(m);
    }
    // several devices: dynamic ready queue
    const double t_start = now_s();
    std::mutex qm;
    std::condition_variable cv;
    std::vector<char> queued(m->done.size(), 0), busy(ndev, 0);
    std::vector<std::thread> running(ndev);
    std::vector<int> finished;           // devices whose unit has ended and whose thread can be joined
    int in_flight = 0, err = PAGAN_OK;
    const int per = std::max(1, threads / ndev);
    std::unique_lock<std::mutex> lk(qm);
    for (;;) {
        for (int d : finished) { running[d].join(); busy[d] = 0; }
        finished.clear();
        if (err != PAGAN_OK || (m->remaining == 0 && in_flight == 0)) break;
        std::vector<int> ready, idle;
        for (int id = m->n_leaves; id < 2 * m->n_leaves - 1; ++id) if (!queued[id] && node_ready(m, id)) ready.push_back(id);
        for (int d = 0; d < ndev; ++d) if (!busy[d]) idle.push_back(d);
        if (!ready.empty() && !idle.empty()) {
            std::vector<int64_t> cost(ready.size());
            for (size_t k = 0; k < ready.size(); ++k) cost[k] = node_cost_estimate(m, ready[k]);
            const int workers = (int)std::min(idle.size(), ready.size());
            std::vector<int32_t> owner(ready.size());
            pagan_assign_units((int32_t)ready.size(), cost.data(), workers, owner.data());
            const int round = m->rounds++;
            for (int w = 0; w < workers; ++w) {
                std::vector<int> mine;
                for (size_t k = 0; k < ready.size(); ++k) if (owner[k] == w) { mine.push_back(ready[k]); queued[ready[k]] = 1; }
                const int d = idle[w];
                busy[d] = 1; ++in_flight;
                running[d] = std::thread([&, d, mine, round] {
                    const int rc = run_unit(m, mine, first_dev + d, round, per, sw);
                    std::lock_guard<std::mutex> g(qm);
                    if (rc != PAGAN_OK && err == PAGAN_OK) err = rc;
                    if (rc == PAGAN_OK) for (int id : mine) { m->done[id] = 1; --m->remaining; }
                    --in_flight; finished.push_back(d);
                    cv.notify_all();
                });
            }
            continue;
        }
        if (in_flight == 0) { err = PAGAN_E_INTERNAL; break; }
        cv.wait(lk);
    }
    while (in_flight > 0) cv.wait(lk);
    for (int d : finished) running[d].join();
    lk.unlock();
    if (err != PAGAN_OK) return err;
    m->tm.total_s += now_s() - t_start;
    return pagan_msa_finish(m);
}

// ---- results across processes (one rank per GPU): what a node's alignment left behind, as bytes ------------
// Layout: int32 magic, node, status, end_matrix, end_x, end_y, end_x_edge, end_y_edge, n_cols, n_left_used,
// n_right_used, packed; int64 cells; double score; then the columns -- packed: one byte of path_state per column
// (the child indices are running counters, basic_alignment.cpp:73-165), else int32 triples -- and the used edge ids.
static const int32_t kResultMagic = 0x50475232;   // "PGR2"

int64_t pagan_msa_export_result(const pagan_msa *m, int32_t id, void *buf, int64_t cap) {
    const NodeWork *w = m ? node_with(m, id - m->n_leaves, kRes) : nullptr;
    if (!w) return PAGAN_E_ARG;
    const pagan_result &r = w->job.res.get();
    bool packed = true;
    {
        int l = 1, rr = 1;
        for (int k = 0; k < r.n_cols && packed; ++k) {
            const pagan_col &c = r.cols[k];
            const bool hl = c.path_state == PAGAN_MATCHED || c.path_state == PAGAN_XGAPPED || c.path_state == PAGAN_XSKIPPED;
            const bool hr = c.path_state == PAGAN_MATCHED || c.path_state == PAGAN_YGAPPED || c.path_state == PAGAN_YSKIPPED;
            if ((hl ? c.left != l : c.left != -1) || (hr ? c.right != rr : c.right != -1)) packed = false;
            l += hl; rr += hr;
        }
    }
    const int64_t need = 12 * 4 + 8 + 8 + (packed ? (int64_t)r.n_cols : 12 * (int64_t)r.n_cols) + 4 * ((int64_t)r.n_left_used + r.n_right_used);
    if (!buf || cap < need) return need;
    char *p = (char *)buf;
    const int32_t head[12] = {kResultMagic, id, r.status, r.end_matrix, r.end_x, r.end_y, r.end_x_edge, r.end_y_edge,
                              r.n_cols, r.n_left_used, r.n_right_used, packed ? 1 : 0};
    std::memcpy(p, head, sizeof(head)); p += sizeof(head);
    std::memcpy(p, &r.cells, 8); p += 8;
    std::memcpy(p, &r.score, 8); p += 8;
    if (packed) for (int k = 0; k < r.n_cols; ++k) *p++ = (char)r.cols[k].path_state;
    else { std::memcpy(p, r.cols, 12 * (size_t)r.n_cols); p += 12 * (size_t)r.n_cols; }
    if (r.n_left_used) std::memcpy(p, r.left_used, 4 * (size_t)r.n_left_used);
    p += 4 * (size_t)r.n_left_used;
    if (r.n_right_used) std::memcpy(p, r.right_used, 4 * (size_t)r.n_right_used);
    return need;
}

// Takes over a node aligned by another rank: stores the result and marks the node done.  The parent graph is NOT built here
// (round 5; before, every rank built every parent, on the one thread that drains the posting log): ensure_graph builds it
// when this process claims a node above it or is asked for the rows.
int pagan_msa_import_result(pagan_msa *m, const void *buf, int64_t bytes) {
    if (!m || !buf || bytes < 12 * 4 + 16) return PAGAN_E_ARG;
    const char *p = (const char *)buf;
    int32_t head[12];
    std::memcpy(head, p, sizeof(head)); p += sizeof(head);
    if (head[0] != kResultMagic) return PAGAN_E_ARG;
    const int id = head[1];
    if (id < m->n_leaves || id >= 2 * m->n_leaves - 1 || !node_ready(m, id)) return PAGAN_E_ARG;
    const int n_cols = head[8], nl = head[9], nr = head[10], packed = head[11];
    if (n_cols < 0 || nl < 0 || nr < 0) return PAGAN_E_ARG;
    const int64_t need = 12 * 4 + 16 + (packed ? (int64_t)n_cols : 12 * (int64_t)n_cols) + 4 * ((int64_t)nl + nr);
    if (bytes < need) return PAGAN_E_ARG;
    NodeWork &w = m->work[id - m->n_leaves];
    w.job.res.reset();
    pagan_result r{};
    r.status = head[2]; r.end_matrix = head[3]; r.end_x = head[4]; r.end_y = head[5]; r.end_x_edge = head[6]; r.end_y_edge = head[7];
    r.n_cols = n_cols; r.n_left_used = nl; r.n_right_used = nr;
    std::memcpy(&r.cells, p, 8); p += 8;
    std::memcpy(&r.score, p, 8); p += 8;
    // the owner releases these with free(), on every return from here on (it reaches the node only when the payload is good)
    r.cols = (pagan_col *)std::malloc(sizeof(pagan_col) * (size_t)std::max(n_cols, 1));
    r.left_used = (int32_t *)std::malloc(4 * (size_t)std::max(nl, 1));
    r.right_used = (int32_t *)std::malloc(4 * (size_t)std::max(nr, 1));
    OwnedResult in;
    in.adopt(r);
    if (!r.cols || !r.left_used || !r.right_used) return PAGAN_E_NOMEM;
    if (packed) {
        int l = 1, rr = 1;
        for (int k = 0; k < n_cols; ++k) {
            const int ps = (unsigned char)*p++;
            const bool hl = ps == PAGAN_MATCHED || ps == PAGAN_XGAPPED || ps == PAGAN_XSKIPPED;
            const bool hr = ps == PAGAN_MATCHED || ps == PAGAN_YGAPPED || ps == PAGAN_YSKIPPED;
            r.cols[k].path_state = ps; r.cols[k].left = hl ? l++ : -1; r.cols[k].right = hr ? rr++ : -1;
        }
    } else { std::memcpy(r.cols, p, 12 * (size_t)n_cols); p += 12 * (size_t)n_cols; }
    if (nl) std::memcpy(r.left_used, p, 4 * (size_t)nl);
    p += 4 * (size_t)nl;
    if (nr) std::memcpy(r.right_used, p, 4 * (size_t)nr);
    // What can be checked without the child graphs is checked now: the path states, and that a column names a child site
    // exactly where its state says it has one.  The rest -- the sites against the children's sizes, the used edges against
    // their edge lists -- when the parent graph is built (ensure_graph), which happens when this process needs it: when it
    // claims a node above, or is asked for the rows.  Nothing of the payload is used as an index before that.
    const TreeNode &t = m->tree[m->tree_of_id[id]];
    bool good = r.status == PAGAN_DP_REACHED || r.status == PAGAN_DP_UNREACHABLE;
    for (int k = 0; good && k < n_cols; ++k) {
        const pagan_col &c = r.cols[k];
        if (c.path_state < PAGAN_MATCHED || c.path_state > PAGAN_YSKIPPED) { good = false; break; }
        const bool hl = c.path_state == PAGAN_MATCHED || c.path_state == PAGAN_XGAPPED || c.path_state == PAGAN_XSKIPPED;
        const bool hr = c.path_state == PAGAN_MATCHED || c.path_state == PAGAN_YGAPPED || c.path_state == PAGAN_YSKIPPED;
        if (hl ? c.left < 1 : c.left != -1) good = false;
        if (hr ? c.right < 1 : c.right != -1) good = false;
    }
    if (!good) return PAGAN_E_ARG;
    w.job.res = std::move(in);
    w.has_job = false; w.device = -1; w.node = id; w.level = m->rounds;
    w.has_fb = false; w.has_marg = false;                          // (support is not part of the exchange format)
    w.imp_l = sites_of(m, m->id_of_tree[t.left]); w.imp_r = sites_of(m, m->id_of_tree[t.right]);   // (no job was prepared here: node_info reports the children's sizes from these)
    if (r.status != PAGAN_DP_REACHED) return PAGAN_E_INTERNAL;       // (the owner retries an unreachable corner itself: it never posts one)
    w.parent_pending = true;
    m->done[id] = 1; --m->remaining;
    return PAGAN_OK;
}

int pagan_msa_n_internal(const pagan_msa *m) { return m ? m->n_leaves - 1 : 0; }

int pagan_msa_node_info(const pagan_msa *m, int32_t k, pagan_node_info *o) {
    const NodeWork *wp = node_with(m, k, kAny);
    if (!wp || !o) return PAGAN_E_ARG;
    const NodeWork &w = *wp;
    const pagan_result &res = w.job.res.get();
    const int id = m->n_leaves + k;
    const TreeNode &t = m->tree[m->tree_of_id[id]];
    std::memset(o, 0, sizeof(*o));
    o->node = id; o->left = m->id_of_tree[t.left]; o->right = m->id_of_tree[t.right];
    o->level = w.level; o->n_hits = w.n_hits; o->n_forced_gaps = w.n_forced;
    o->dist = m->tree[t.left].dist + m->tree[t.right].dist;
    if (w.job.res.held()) {
        o->left_sites = w.has_job ? w.job.gl.n_sites : w.imp_l; o->right_sites = w.has_job ? w.job.gr.n_sites : w.imp_r;
        o->cells = res.cells; o->score = res.score; o->status = res.status;
    }
    if (m->graph[id]) o->sites = m->graph[id]->g.n_sites();
    return PAGAN_OK;
}

int pagan_msa_node_job(const pagan_msa *m, int32_t k, pagan_job *o) {
    const NodeWork *w = node_with(m, k, kRes | kJob);
    if (!w || !o) return PAGAN_E_ARG;
    *o = w->job.job(&w->pm);
    return PAGAN_OK;
}

int pagan_msa_node_result(const pagan_msa *m, int32_t k, pagan_result *o) {
    const NodeWork *w = node_with(m, k, kRes);
    if (!w || !o) return PAGAN_E_ARG;
    *o = w->job.res.get();                                          // (a borrowed shallow copy: the node keeps the arrays)
    return PAGAN_OK;
}

// ---- what the forward/backward pass left at a node (full_probability / sample_path); PAGAN_E_ARG for a node this process
// did not align
int pagan_msa_node_fb(const pagan_msa *m, int32_t k, double out[4]) {
    const NodeWork *w = node_with(m, k, kFb);
    if (!w || !out) return PAGAN_E_ARG;
    out[0] = w->log_fwd; out[1] = w->log_bwd; out[2] = w->fb_sweep_ms; out[3] = w->fb_post_ms;
    return PAGAN_OK;
}

// ... and the posterior decoding (pagan_msa_set_decoder)
int pagan_msa_node_decode(const pagan_msa *m, int32_t k, double out[3]) {
    const NodeWork *w = node_with(m, k, kDec);
    if (!w || !out) return PAGAN_E_ARG;
    out[0] = w->dec_objective; out[1] = w->dec_steps; out[2] = w->dec_ms;
    return PAGAN_OK;
}

// ... and the expected counts (pagan_msa_set_counts): trans[12], emit[S * S] (DNA; NULL: not wanted)
int pagan_msa_node_counts(const pagan_msa *m, int32_t k, double *trans, double *emit) {
    const NodeWork *w = node_with(m, k, kFb | kCounts);
    if (!w || !trans) return PAGAN_E_ARG;
    if (emit && w->emit.empty()) return PAGAN_E_ARG;                // (protein and codon tables: not provided)
    std::memcpy(trans, w->trans, sizeof(w->trans));
    if (emit) std::memcpy(emit, w->emit.data(), 8 * w->emit.size());
    return PAGAN_OK;
}

int pagan_msa_node_support(const pagan_msa *m, int32_t k, double *support) {
    const NodeWork *w = node_with(m, k, kFb);
    if (!w || !support) return PAGAN_E_ARG;
    if (!w->support.empty()) std::memcpy(support, w->support.data(), 8 * w->support.size());
    return PAGAN_OK;
}

int pagan_msa_node_marginals(const pagan_msa *m, int32_t k, double *pX, double *pM_left, int32_t *best_j, double *best_p_left,
                             double *pY, double *pM_right, int32_t *best_i, double *best_p_right) {
    const NodeWork *w = node_with(m, k, kFb | kMarg);
    if (!w) return PAGAN_E_ARG;
    double *const d[6] = {pX, pM_left, best_p_left, pY, pM_right, best_p_right};
    int32_t *const i[2] = {best_j, best_i};
    for (int a = 0; a < 6; ++a) if (d[a] && !w->mg_d[a].empty()) std::memcpy(d[a], w->mg_d[a].data(), 8 * w->mg_d[a].size());
    for (int a = 0; a < 2; ++a) if (i[a] && !w->mg_i[a].empty()) std::memcpy(i[a], w->mg_i[a].data(), 4 * w->mg_i[a].size());
    return PAGAN_OK;
}

int pagan_msa_node_model_prob(const pagan_msa *m, int32_t k, pagan_model_prob *out) {
    const NodeWork *w = node_with(m, k, kJob);
    if (!w || !out || !w->model) return PAGAN_E_ARG;
    *out = w->model->prob_view();
    return PAGAN_OK;
}

int pagan_msa_timing_get(const pagan_msa *m, pagan_msa_timing *o) {
    if (!m || !o) return PAGAN_E_ARG;
    *o = m->tm;
    return PAGAN_OK;
}

void pagan_msa_destroy(pagan_msa *m) { delete m; }

long long pagan_parents_device_calls(void) { return parents_on_device.load(); }

int pagan_msa_set_batch_backend(pagan_msa *m, pagan_batch_fn fn, void *user) {
    if (!m) return PAGAN_E_ARG;
    m->backend = fn; m->backend_user = user;
    return PAGAN_OK;
}

int pagan_msa_set_sampler(pagan_msa *m, int32_t on_device) {
    if (!m || (on_device != 0 && on_device != 1)) return PAGAN_E_ARG;
    m->sample_on_device = on_device;
    return PAGAN_OK;
}

int pagan_msa_set_decoder(pagan_msa *m, int32_t on, double gap_weight) {
    if (!m || (on != 0 && on != 1) || !(gap_weight >= 0.0) || !(gap_weight < HUGE_VAL)) return PAGAN_E_ARG;
    m->decode_on = on; m->decode_gap = gap_weight;
    return PAGAN_OK;
}

int pagan_msa_set_counts(pagan_msa *m, int32_t on) {
    if (!m || (on != 0 && on != 1)) return PAGAN_E_ARG;
    m->counts_on = on;
    return PAGAN_OK;
}

// Before aligning: a negative value keeps the data type's default.  Both model views follow (ModelFactory::alignment_model reads
// these fields); pileup_rates still replaces the two rates where it applies.
int pagan_msa_set_indel_model(pagan_msa *m, double ins_rate, double del_rate, double gap_ext, double end_gap_ext) {
    if (!m || m->aligned || m->rounds > 0) return PAGAN_E_ARG;
    if (ins_rate != ins_rate || del_rate != del_rate || gap_ext != gap_ext || end_gap_ext != end_gap_ext) return PAGAN_E_ARG;
    if (gap_ext >= 1.0 || gap_ext == 0.0 || end_gap_ext >= 1.0 || end_gap_ext == 0.0) return PAGAN_E_ARG;   // (a probability in (0, 1))
    if ((ins_rate >= 0 || del_rate >= 0) && !((ins_rate >= 0 ? (float)ins_rate : m->mf.ins_rate) + (del_rate >= 0 ? (float)del_rate : m->mf.del_rate) > 0.0f)) return PAGAN_E_ARG;
    if (ins_rate >= 0) { m->mf.ins_rate = (float)ins_rate; m->indel_set = true; }
    if (del_rate >= 0) { m->mf.del_rate = (float)del_rate; m->indel_set = true; }
    if (gap_ext > 0) m->mf.ext_prob = (float)gap_ext;
    if (end_gap_ext > 0) m->mf.end_ext_prob = (float)end_gap_ext;
    std::lock_guard<std::mutex> g(m->mu);
    m->model_cache.clear();
    return PAGAN_OK;
}

int pagan_msa_node_device(const pagan_msa *m, int32_t k) {
    const NodeWork *w = node_with(m, k, kAny);
    return w ? w->device : PAGAN_E_ARG;
}

int pagan_msa_data_type(const pagan_msa *m) { return m ? (m->mf.type == kCodon ? 3 : m->mf.type == kProtein ? 2 : 1) : PAGAN_E_ARG; }

} // extern "C"
