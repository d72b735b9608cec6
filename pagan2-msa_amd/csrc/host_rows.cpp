// host_rows.cpp -- everything that needs the walk's finished alignment: the rows, the FASTA writers, a node's support on the
// alignment's columns, the guide tree and the ancestral states made from the rows, a node's graph on demand.
#include <cstdio>

#include "host_msa.h"

using namespace pagan;

namespace {

void build_rows(pagan_msa *m) {
    const int n = m->n_leaves;
    const int root_id = m->id_of_tree[m->root];
    const int width = m->graph[root_id]->g.n_sites() - 2;
    // a node's column map: site -> column of the alignment (-1: none).  Storage that the host's threads touch first (round 5:
    // the maps' 27 MB and the rows' 8 MB of a 32 x 100 kb walk, allocated and filled by one thread, were most of this function's time)
    std::vector<std::unique_ptr<int32_t[]>> col(m->graph.size());
    col[root_id].reset(new int32_t[width + 2]);
    for (int s = 0; s < width + 2; ++s) col[root_id][s] = s - 1;
    const int w = m->mf.type == kCodon ? 3 : 1;                 // characters per column ("---" gaps for codons)
    m->rows.assign(m->graph.size(), std::string());
    const std::string &anc = m->mf.type == kCodon ? m->mf.codon_names : m->mf.ancestral_alphabet;
    // A node's columns follow from its parent's: the tree is walked by DEPTH, the nodes of one depth side by side on the
    // host's threads (round 5: one thread walking all 2n - 1 nodes was 25 ms of a 0.7 s walk of 32 x 100 kb).
    std::vector<std::vector<int>> by_depth;
    {
        std::vector<std::pair<int, int>> stack{{m->root, 0}};      // (tree index, depth)
        while (!stack.empty()) {
            const auto [t, depth] = stack.back();
            stack.pop_back();
            if ((int)by_depth.size() <= depth) by_depth.resize(depth + 1);
            by_depth[depth].push_back(m->id_of_tree[t]);
            const TreeNode &tn = m->tree[t];
            if (tn.left >= 0) { stack.push_back({tn.left, depth + 1}); stack.push_back({tn.right, depth + 1}); }
        }
    }
    const int threads = host_threads_of(m);
    parallel_for((int)m->rows.size(), threads, [&](int id) { m->rows[id].assign((size_t)width * w, '-'); });
    for (const std::vector<int> &ids : by_depth) {
        // the upper depths hold 1, 2, 4 nodes of 10^5 sites each: a node's sites in `parts` ranges (every site writes its own
        // column of its own row and its own entries of the children's column maps)
        const int parts = std::max(1, std::min(threads, (2 * threads) / std::max(1, (int)ids.size())));
        std::vector<int> kids;
        for (int id : ids)
            if (id >= n) {
                const TreeNode &t = m->tree[m->tree_of_id[id]];
                for (int kid : {m->id_of_tree[t.left], m->id_of_tree[t.right]}) {
                    if (kid < n) continue;                     // (a leaf has no map: its parent writes the leaf's row, below)
                    col[kid].reset(new int32_t[m->graph[kid]->g.n_sites()]);
                    kids.push_back(kid);
                }
            }
        parallel_for((int)kids.size() * parts, threads, [&](int task) {
            const int kid = kids[task / parts], part = task % parts, ns = m->graph[kid]->g.n_sites();
            std::fill(col[kid].get() + (long long)ns * part / parts, col[kid].get() + (long long)ns * (part + 1) / parts, -1);
        });
        parallel_for((int)ids.size() * parts, threads, [&](int task) {
            const int id = ids[task / parts], part = task % parts;
            const SeqGraph &g = m->graph[id]->g;
            std::string &row = m->rows[id];
            const int32_t *mine = col[id].get();
            const int n_in = g.n_sites() - 2;                      // sites 1 .. n_in
            const int s_first = 1 + (int)((long long)n_in * part / parts), s_last = 1 + (int)((long long)n_in * (part + 1) / parts);
            if (id < n) {                                          // a leaf: its residues at its columns (only a tree of one leaf comes here)
                if (!mine) return;
                for (int s = s_first; s < s_last; ++s)
                    for (int c = 0; c < w; ++c) row[(size_t)mine[s] * w + c] = g.symbols[(size_t)(s - 1) * w + c];
                return;
            }
            const TreeNode &t = m->tree[m->tree_of_id[id]];
            const int lid = m->id_of_tree[t.left], rid = m->id_of_tree[t.right];
            int32_t *cl = col[lid].get(), *cr = col[rid].get();
            // a child that is a leaf has no map of its own (half of a tree's nodes, and of the maps' pages): its residues go to
            // its row from here, site c of the leaf at this site's column
            const SeqGraph *gl = lid < n ? &m->graph[lid]->g : nullptr, *gr = rid < n ? &m->graph[rid]->g : nullptr;
            std::string *rl = lid < n ? &m->rows[lid] : nullptr, *rr = rid < n ? &m->rows[rid] : nullptr;
            for (int s = s_first; s < s_last; ++s) {
                const int a = g.child_l[s], b = g.child_r[s];
                if (a >= 0) {
                    if (gl) { for (int c = 0; c < w; ++c) (*rl)[(size_t)mine[s] * w + c] = gl->symbols[(size_t)(a - 1) * w + c]; }
                    else cl[a] = mine[s];
                }
                if (b >= 0) {
                    if (gr) { for (int c = 0; c < w; ++c) (*rr)[(size_t)mine[s] * w + c] = gr->symbols[(size_t)(b - 1) * w + c]; }
                    else cr[b] = mine[s];
                }
                // the ancestor's own row (get_alignment_column_at with include_internal_nodes, node.cpp:808-818): its
                // state's character, a gap where the site is skipped or was deleted
                const int ps = g.path_state[s];
                if (!(ps == PAGAN_XSKIPPED || ps == PAGAN_YSKIPPED || g.site_type[s] == kNonReal) && g.state[s] >= 0)
                    for (int c = 0; c < w; ++c) row[(size_t)mine[s] * w + c] = anc[(size_t)g.state[s] * w + c];
            }
        });
        for (int id : ids) col[id].reset();
    }
}

// the rows on first use (pagan_msa_finish_lazy), from an accessor: the switches are read here, on the caller's thread
int rows_of(const pagan_msa *m) { return ensure_rows(const_cast<pagan_msa *>(m), HostSwitches::read()); }

} // namespace

// The rows of the alignment need every node's graph (an ancestor's row is read off its sites; the leaves' columns follow
// the child maps down from the root): parents still pending (imported nodes, rank mode) are built first.
int pagan::ensure_rows(pagan_msa *m, const HostSwitches &sw) {
    std::lock_guard<std::mutex> g(m->lazy_mu);
    if (m->rows_built) return PAGAN_OK;
    const double t0 = now_s();
    const int rc = ensure_graph(m, m->id_of_tree[m->root]);
    if (rc != PAGAN_OK) return rc;
    const double t1 = now_s();
    build_rows(m);
    m->tm.total_s += now_s() - t0;
    if (sw.verbose)
        std::fprintf(stderr, "pagan_msa: finish: pending parents %.1f ms, rows %.1f ms\n", 1e3 * (t1 - t0), 1e3 * (now_s() - t1));
    m->rows_built = true;
    return PAGAN_OK;
}

extern "C" {

// A node's column support on the columns of the final alignment: the node's sites are followed up the tree, parent by parent,
// to the root's sites, which are the alignment's columns (as build_rows follows them down).
int pagan_msa_support_row(const pagan_msa *m, int32_t node, float *buf) {
    if (!m || !m->aligned || !buf) return PAGAN_E_ARG;
    if (node < m->n_leaves || node >= 2 * m->n_leaves - 1 || !m->work[node - m->n_leaves].has_fb) return PAGAN_E_ARG;
    if (const int rc = rows_of(m)) return rc;
    const NodeWork &w = m->work[node - m->n_leaves];
    const pagan_result &res = w.job.res.get();
    const int width = (int)m->rows[0].size() / (m->mf.type == kCodon ? 3 : 1);
    for (int c = 0; c < width; ++c) buf[c] = -1.0f;
    const int ns = m->graph[node]->g.n_sites();
    if (ns != res.n_cols + 2 || (int)w.support.size() != res.n_cols) return PAGAN_E_INTERNAL;
    std::vector<int32_t> at(ns);                                   // site of `node` -> site of the ancestor reached so far
    for (int s = 0; s < ns; ++s) at[s] = s;
    for (int t = m->tree_of_id[node]; m->tree[t].parent >= 0; t = m->tree[t].parent) {
        const int pt = m->tree[t].parent;
        const SeqGraph &pg = m->graph[m->id_of_tree[pt]]->g;
        const std::vector<int32_t> &child = m->tree[pt].left == t ? pg.child_l : pg.child_r;
        std::vector<int32_t> up((size_t)m->graph[m->id_of_tree[t]]->g.n_sites(), -1);
        for (int s = 1; s < pg.n_sites() - 1; ++s) if (child[s] >= 0) up[child[s]] = s;
        for (int s = 1; s < ns - 1; ++s) if (at[s] >= 0) at[s] = up[at[s]];
    }
    for (int k = 0; k < res.n_cols; ++k) {
        const int ps = res.cols[k].path_state;
        if (ps != PAGAN_MATCHED && ps != PAGAN_XGAPPED && ps != PAGAN_YGAPPED) continue;
        const int c = at[k + 1] - 1;                               // (the root's site s is column s - 1)
        if (c >= 0 && c < width) buf[c] = (float)w.support[k];
    }
    return PAGAN_OK;
}

int pagan_msa_alignment_length(const pagan_msa *m) {
    if (!m || !m->aligned) return PAGAN_E_ARG;
    if (const int rc = rows_of(m)) return rc;                      // (pagan_msa_finish_lazy: built on first use)
    return (int)m->rows[0].size();
}

int pagan_msa_alignment_row(const pagan_msa *m, int32_t leaf, char *buf) {
    if (!m || !m->aligned || !buf) return PAGAN_E_ARG;
    if (const int rc = rows_of(m)) return rc;
    if (leaf < 0 || leaf >= (int)m->rows.size()) return PAGAN_E_ARG;
    std::memcpy(buf, m->rows[leaf].c_str(), m->rows[leaf].size() + 1);
    return PAGAN_OK;
}

// The guide tree made from this walk's own alignment (csrc/dp_alndist.hip): the leaf rows, the walk's names and data type.
int64_t pagan_msa_alignment_tree(const pagan_msa *m, char *newick_out, int64_t cap, pagan_aln_info *info) {
    if (!m || !m->aligned || (cap > 0 && !newick_out)) return PAGAN_E_ARG;
    if (const int rc = rows_of(m)) return rc;
    std::vector<const char *> names(m->n_leaves), rows(m->n_leaves);
    for (int k = 0; k < m->n_leaves; ++k) { names[k] = m->names[k].c_str(); rows[k] = m->rows[k].c_str(); }
    return pagan_aln_tree(m->n_leaves, names.data(), rows.data(), pagan_msa_data_type(m), newick_out, cap, info);
}

// Fasta_reader::write_fasta (src/utils/fasta_reader.cpp:596-629) over Node::get_alignment's leaf rows
// (src/main/node.cpp:537-575): one entry per leaf in guide-tree order (left to right, as get_leaf_nodes
// collects them), `>name`, the aligned row cut into lines of chars_by_line characters (60 by default).
int pagan_msa_write_fasta(const pagan_msa *m, const char *path, int32_t chars_by_line) {
    return pagan_msa_write_fasta_nodes(m, path, chars_by_line, 0);
}

// ... with include_internal (--output-ancestors): every node in Node::get_all_nodes order -- left subtree, the node,
// right subtree (node.h:277-290) -- internal nodes named #k# in alignment order (node.h:479-495).
static int write_fasta_rows(const pagan_msa *m, const std::vector<std::string> &rows, const char *path, int32_t chars_by_line, int32_t include_internal) {
    const size_t width = chars_by_line > 0 ? (size_t)chars_by_line : 60;
    std::FILE *f = std::fopen(path, "w");
    if (!f) return PAGAN_E_ARG;
    std::vector<int> order;
    {
        // in-order walk without recursion: (tree index, children done?)
        std::vector<std::pair<int, bool>> stack{{m->root, false}};
        while (!stack.empty()) {
            const auto [t, visited] = stack.back();
            stack.pop_back();
            const TreeNode &n = m->tree[t];
            if (n.left < 0) { order.push_back(m->id_of_tree[t]); continue; }
            if (visited) { if (include_internal) order.push_back(m->id_of_tree[t]); continue; }
            stack.push_back({n.right, false});
            stack.push_back({t, true});
            stack.push_back({n.left, false});
        }
    }
    for (int leaf : order) {
        if (leaf < m->n_leaves) std::fprintf(f, ">%s\n", m->names[leaf].c_str());
        else std::fprintf(f, ">#%d#\n", leaf - m->n_leaves + 1);
        const std::string &row = rows[leaf];
        for (size_t at = 0; at < row.size(); at += width) std::fprintf(f, "%.*s\n", (int)std::min(width, row.size() - at), row.c_str() + at);
    }
    return std::fclose(f) == 0 ? PAGAN_OK : PAGAN_E_ARG;
}

int pagan_msa_write_fasta_nodes(const pagan_msa *m, const char *path, int32_t chars_by_line, int32_t include_internal) {
    if (!m || !m->aligned || !path) return PAGAN_E_ARG;
    if (const int rc = rows_of(m)) return rc;
    return write_fasta_rows(m, m->rows, path, chars_by_line, include_internal);
}

// ---- ancestral states by marginal likelihood (csrc/dp_anc.hip) over the finished walk -----------------------------------
// The walk's tree in its public ids (children before parents, the root 2n - 2) under the branch lengths it aligned with:
// tree[].dist after corrected_branch.
int pagan_msa_ancestral(pagan_msa *m, uint32_t flags, double *loglik, double *col_loglik, pagan_anc_info *info) {
    if (!m || !m->aligned) return PAGAN_E_ARG;
    if (const int rc = rows_of(m)) return rc;
    try {
        const int n = m->n_leaves;
        std::vector<int32_t> left(n - 1), right(n - 1);
        std::vector<double> branch((size_t)2 * n - 1, 0.0);
        std::vector<const char *> rows(n);
        for (int k = 0; k < n - 1; ++k) {
            const TreeNode &t = m->tree[m->tree_of_id[n + k]];
            left[k] = m->id_of_tree[t.left]; right[k] = m->id_of_tree[t.right];
        }
        for (int id = 0; id < 2 * n - 1; ++id) branch[id] = m->tree[m->tree_of_id[id]].dist;
        for (int k = 0; k < n; ++k) rows[k] = m->rows[k].c_str();
        float bf[4] = {0.25f, 0.25f, 0.25f, 0.25f};
        if (m->mf.type == kDna) for (int k = 0; k < 4; ++k) bf[k] = (float)m->mf.pi[k];     // (the floats init_dna took)
        const size_t L = m->rows[0].size() / (m->mf.type == kCodon ? 3 : 1);
        std::vector<uint8_t> best((size_t)(n - 1) * L);
        std::vector<float> best_p((size_t)(n - 1) * L);
        m->anc_done = false;
        const int rc = pagan_anc_reconstruct(n, left.data(), right.data(), branch.data(), rows.data(), pagan_msa_data_type(m), bf, flags, 0, nullptr,
                                             nullptr, nullptr, col_loglik, loglik, best.data(), best_p.data(), nullptr, nullptr, info);
        if (rc != PAGAN_OK) return rc;
        m->anc_best.swap(best); m->anc_best_p.swap(best_p);
        m->anc_done = true;
        return PAGAN_OK;
    } catch (const std::bad_alloc &) {
        return PAGAN_E_NOMEM;
    }
}

// The overlay of bppancestors.cpp:242-254: every character of an ancestor's row that is no gap becomes the state of largest
// posterior; the root keeps its own (no copy from a child as at :273-314: the pass is rooted).
static std::string ancestral_row_of(const pagan_msa *m, int node) {
    std::string row = m->rows[node];
    const int n = m->n_leaves;
    if (node < n) return row;
    const int w = m->mf.type == kCodon ? 3 : 1;
    const size_t L = row.size() / w;
    const char *letters = m->mf.type == kCodon ? ModelFactory::codon_alphabet() : m->mf.type == kProtein ? ModelFactory::protein_alphabet() : ModelFactory::dna_full_alphabet();
    const uint8_t *best = m->anc_best.data() + (size_t)(node - n) * L;
    for (size_t c = 0; c < L; ++c)
        if (row[c * w] != '-') for (int j = 0; j < w; ++j) row[c * w + j] = letters[(size_t)best[c] * w + j];
    return row;
}

int pagan_msa_ancestral_row(const pagan_msa *m, int32_t node, char *buf) {
    if (!m || !m->aligned || !m->anc_done || !buf || node < 0 || node >= (int)m->rows.size()) return PAGAN_E_ARG;
    const std::string row = ancestral_row_of(m, node);
    std::memcpy(buf, row.c_str(), row.size() + 1);
    return PAGAN_OK;
}

int pagan_msa_ancestral_support(const pagan_msa *m, int32_t node, float *buf) {
    if (!m || !m->aligned || !m->anc_done || !buf || node < m->n_leaves || node >= (int)m->rows.size()) return PAGAN_E_ARG;
    const int w = m->mf.type == kCodon ? 3 : 1;
    const std::string &row = m->rows[node];
    const size_t L = row.size() / w;
    const float *p = m->anc_best_p.data() + (size_t)(node - m->n_leaves) * L;
    for (size_t c = 0; c < L; ++c) buf[c] = row[c * w] != '-' ? p[c] : -1.0f;
    return PAGAN_OK;
}

int pagan_msa_write_fasta_ancestral(const pagan_msa *m, const char *path, int32_t chars_by_line) {
    if (!m || !m->aligned || !m->anc_done || !path) return PAGAN_E_ARG;
    try {
        std::vector<std::string> rows(m->rows.size());
        for (size_t id = 0; id < rows.size(); ++id) rows[id] = ancestral_row_of(m, (int)id);
        return write_fasta_rows(m, rows, path, chars_by_line, 1);
    } catch (const std::bad_alloc &) {
        return PAGAN_E_NOMEM;
    }
}

int pagan_msa_ancestral_best(const pagan_msa *m, const uint8_t **best, const float **best_p) {
    if (!m || !m->anc_done) return PAGAN_E_ARG;
    if (best) *best = m->anc_best.data();
    if (best_p) *best_p = m->anc_best_p.data();
    return PAGAN_OK;
}

// ---- branch lengths by maximum likelihood (csrc/dp_anc_brlen.inc) over the finished walk ----------------------------------
// pagan_msa_ancestral's inputs -- the walk's tree in its public ids, the lengths it aligned under, its rows and base
// frequencies -- and a Newick of the same topology and names with the fitted lengths.
int64_t pagan_msa_fit_branches(const pagan_msa *m, const pagan_anc_fit_opts *opts, double *branch_out, char *newick_out, int64_t cap,
                               pagan_anc_fit_info *info) {
    if (!m || !m->aligned || (cap > 0 && !newick_out)) return PAGAN_E_ARG;
    if (const int rc = rows_of(m)) return rc;
    try {
        const int n = m->n_leaves;
        std::vector<int32_t> left(n - 1), right(n - 1);
        std::vector<double> branch((size_t)2 * n - 1, 0.0), fitted((size_t)2 * n - 1, 0.0);
        std::vector<const char *> rows(n);
        for (int k = 0; k < n - 1; ++k) {
            const TreeNode &t = m->tree[m->tree_of_id[n + k]];
            left[k] = m->id_of_tree[t.left]; right[k] = m->id_of_tree[t.right];
        }
        for (int id = 0; id < 2 * n - 1; ++id) branch[id] = m->tree[m->tree_of_id[id]].dist;
        for (int k = 0; k < n; ++k) rows[k] = m->rows[k].c_str();
        float bf[4] = {0.25f, 0.25f, 0.25f, 0.25f};
        if (m->mf.type == kDna) for (int k = 0; k < 4; ++k) bf[k] = (float)m->mf.pi[k];
        const int rc = pagan_anc_fit_branches(n, left.data(), right.data(), branch.data(), rows.data(), pagan_msa_data_type(m), bf, opts,
                                              fitted.data(), nullptr, 0, info);
        if (rc < 0) return rc;
        if (branch_out) std::copy(fitted.begin(), fitted.end(), branch_out);
        // the tree in post-order without recursion: (tree index, children written?)
        std::string out;
        char num[40];
        std::vector<std::pair<int, int>> stack{{m->root, 0}};
        while (!stack.empty()) {
            auto &[t, stage] = stack.back();
            const TreeNode &node = m->tree[t];
            if (node.left >= 0 && stage == 0) { out += '('; stage = 1; stack.push_back({node.left, 0}); continue; }
            if (node.left >= 0 && stage == 1) { out += ','; stage = 2; stack.push_back({node.right, 0}); continue; }
            if (node.left >= 0) out += ')'; else out += node.name;
            if (t != m->root) { std::snprintf(num, sizeof(num), ":%.17g", fitted[m->id_of_tree[t]]); out += num; }
            stack.pop_back();
        }
        out += ';';
        const int64_t need = (int64_t)out.size() + 1;
        if (need <= cap) std::memcpy(newick_out, out.c_str(), (size_t)need);
        return need;
    } catch (const std::bad_alloc &) {
        return PAGAN_E_NOMEM;
    }
}

// ---- tree search by nearest-neighbour interchange (csrc/dp_anc_nni.inc) over the finished walk -----------------------------
// pagan_msa_fit_branches' inputs; the tree found is printed from its arrays, since its topology is no longer the walk's.
int64_t pagan_msa_search_tree(const pagan_msa *m, const pagan_anc_nni_opts *opts, char *newick_out, int64_t cap, pagan_anc_nni_info *info) {
    if (!m || !m->aligned || (cap > 0 && !newick_out)) return PAGAN_E_ARG;
    if (const int rc = rows_of(m)) return rc;
    try {
        const int n = m->n_leaves;
        std::vector<int32_t> left(n - 1), right(n - 1);
        std::vector<double> branch((size_t)2 * n - 1, 0.0);
        std::vector<const char *> rows(n);
        for (int k = 0; k < n - 1; ++k) {
            const TreeNode &t = m->tree[m->tree_of_id[n + k]];
            left[k] = m->id_of_tree[t.left]; right[k] = m->id_of_tree[t.right];
        }
        for (int id = 0; id < 2 * n - 1; ++id) branch[id] = m->tree[m->tree_of_id[id]].dist;
        for (int k = 0; k < n; ++k) rows[k] = m->rows[k].c_str();
        float bf[4] = {0.25f, 0.25f, 0.25f, 0.25f};
        if (m->mf.type == kDna) for (int k = 0; k < 4; ++k) bf[k] = (float)m->mf.pi[k];
        std::vector<int32_t> lo(n - 1), ro(n - 1);
        std::vector<double> bo((size_t)2 * n - 1, 0.0);
        const int rc = pagan_anc_nni_search(n, left.data(), right.data(), branch.data(), rows.data(), pagan_msa_data_type(m), bf, opts, lo.data(),
                                            ro.data(), bo.data(), nullptr, 0, nullptr, 0, nullptr, info);
        if (rc < 0) return rc;
        // children come before parents: a node's text is made of its children's
        std::vector<std::string> text((size_t)2 * n - 1);
        char num[40];
        for (int k = 0; k < n; ++k) text[k] = m->names[k];
        for (int k = 0; k < n - 1; ++k) {
            std::string &out = text[(size_t)n + k];
            out = "(";
            for (const int32_t c : {lo[k], ro[k]}) {
                out += text[c];
                text[c].clear();
                std::snprintf(num, sizeof(num), ":%.17g", bo[c]);
                out += num;
                out += c == lo[k] ? "," : ")";
            }
        }
        const std::string out = text[(size_t)2 * n - 2] + ";";
        const int64_t need = (int64_t)out.size() + 1;
        if (need <= cap) std::memcpy(newick_out, out.c_str(), (size_t)need);
        return need;
    } catch (const std::bad_alloc &) {
        return PAGAN_E_NOMEM;
    }
}

void *pagan_msa_node_graph(const pagan_msa *m, int32_t node) {
    if (!m || node < 0 || node >= (int)m->graph.size()) return nullptr;
    if (!m->graph[node] && m->done[node]) {                        // (an imported node's graph: built when somebody asks for it)
        pagan_msa *mm = const_cast<pagan_msa *>(m);
        std::lock_guard<std::mutex> g(mm->lazy_mu);
        if (ensure_graph(mm, node) != PAGAN_OK) return nullptr;
    }
    return m->graph[node].get();
}

} // extern "C"
