// host_anc.cpp -- the host-only part of the ancestral reconstruction (include/pagan_host.h, "ancestral states by marginal
// likelihood"; DESIGN.md "Ancestral states"): the transition matrices, the leaf tables, the tree check, the chunk size and the
// device layout.  Nothing here needs a device; csrc/dp_anc.hip runs the passes.
#include "host_anc.h"

#include <algorithm>
#include <cctype>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <new>

#include "../../include/pagan_host.h"
#include "dp_pool.h"
#include "host_guide.h"

namespace pagan {

int anc_states(int data_type) { return data_type == 1 ? 4 : data_type == 2 ? 20 : data_type == 3 ? 61 : 0; }

// The factory's eigen solution again, of the model's rate matrix made a proper one.  The reference's matrices are not: the DNA
// rates are float products and the codon rates a table of decimal literals, so detailed balance under pi and the zero row sums
// hold only to the digits those carry, and P(t) of the alignment model has row sums off 1 by up to 1.2e-8 (DNA) and 6.6e-5
// (codons).  That is harmless in a log-odds score table and wrong in a likelihood.  From the model's Q: r_ij =
// (pi_i q_ij + pi_j q_ji) / 2 / pi_i for i != j (each exchange flow averaged with its mirror image), r_ii = -(r_i0 + r_i1 + ...)
// in column order, and eigen_qrev solves that; mf->Q becomes r.  P itself is never renormalised.  False: the solver failed.
static bool anc_proper_rates(ModelFactory *mf) {
    const int n = mf->char_as;
    const std::vector<double> &Q = mf->Q;
    std::vector<double> R((size_t)n * n, 0.0);
    for (int i = 0; i < n; ++i) {
        double off = 0.0;
        for (int j = 0; j < n; ++j) {
            if (j == i) continue;
            R[(size_t)i * n + j] = 0.5 * (mf->pi[i] * Q[(size_t)i * n + j] + mf->pi[j] * Q[(size_t)j * n + i]) / mf->pi[i];
            off += R[(size_t)i * n + j];
        }
        R[(size_t)i * n + i] = -off;
    }
    mf->Q = R;
    return eigen_qrev(R.data(), mf->pi.data(), n, mf->root.data(), mf->U.data(), mf->V.data()) == 0;
}

int anc_factory(int data_type, const float *base_freq, ModelFactory *mf) {
    struct Made { ModelFactory f; bool ok; };
    if (data_type == 1) {
        const float flat[4] = {0.25f, 0.25f, 0.25f, 0.25f};
        mf->init_dna(base_freq ? base_freq : flat);
        return anc_proper_rates(mf) ? PAGAN_OK : PAGAN_E_INTERNAL;
    }
    static const Made protein = [] { Made m; m.f.init_protein(); m.ok = anc_proper_rates(&m.f); return m; }();
    static const Made codon = [] { Made m; m.f.init_codon(); m.ok = anc_proper_rates(&m.f); return m; }();
    const Made &made = data_type == 2 ? protein : codon;
    *mf = made.f;
    return made.ok ? PAGAN_OK : PAGAN_E_INTERNAL;
}

void anc_pmatrix(const ModelFactory &mf, double t, double *P) {
    const int n = mf.char_as;
    if (t == 0) {
        for (int i = 0; i < n; ++i) for (int j = 0; j < n; ++j) P[(size_t)i * n + j] = i == j ? 1.0 : 0.0;
        return;
    }
    std::fill(P, P + (size_t)n * n, 0.0);
    for (int k = 0; k < n; ++k) {                                  // ModelFactory::alignment_model's sum, k outermost, over anc_factory's solution
        const double e1 = std::exp(t * mf.root[k]);
        for (int i = 0; i < n; ++i) {
            const double e2 = mf.U[(size_t)i * n + k] * e1;
            for (int j = 0; j < n; ++j) P[(size_t)i * n + j] += e2 * mf.V[(size_t)k * n + j];
        }
    }
    for (size_t k = 0; k < (size_t)n * n; ++k) P[k] = std::max(0.0, P[k]);
}

void anc_leaf_tables(int data_type, unsigned char table[256], unsigned char triplet[64]) {
    std::memset(table, data_type == 1 ? 0 : kAncMissing, 256);
    std::memset(triplet, kAncMissing, 64);
    auto both_cases = [&](char c, unsigned char v) { table[(unsigned char)c] = table[(unsigned char)std::tolower(c)] = v; };
    if (data_type == 1) {
        // dna_full_alphabet()'s letters as the sets alignment_model lists for them
        static const unsigned char bits[15] = {1, 2, 4, 8, 1 | 4, 2 | 8, 1 | 2, 4 | 8, 1 | 8, 2 | 4, 2 | 4 | 8, 1 | 4 | 8, 1 | 2 | 8, 1 | 2 | 4, 15};
        const char *a = ModelFactory::dna_full_alphabet();
        for (int k = 0; k < 15; ++k) both_cases(a[k], bits[k]);
        both_cases('U', 8);
    } else if (data_type == 2) {
        const char *a = ModelFactory::protein_alphabet();
        for (int k = 0; k < 20; ++k) both_cases(a[k], (unsigned char)k);
    } else {
        const char base[4] = {'A', 'C', 'G', 'T'};
        for (int k = 0; k < 4; ++k) both_cases(base[k], (unsigned char)k);
        both_cases('U', 3);
        const char *names = ModelFactory::codon_alphabet();
        for (int k = 0; k < 61; ++k)
            triplet[table[(unsigned char)names[3 * k]] * 16 + table[(unsigned char)names[3 * k + 1]] * 4 + table[(unsigned char)names[3 * k + 2]]] = (unsigned char)k;
    }
}

int anc_check_tree(int32_t n, const int32_t *left, const int32_t *right, const double *branch) {
    if (n < 2 || !left || !right || !branch) return PAGAN_E_ARG;
    std::vector<char> used((size_t)2 * n - 1, 0);
    for (int k = 0; k < n - 1; ++k)
        for (const int32_t c : {left[k], right[k]}) {
            if (c < 0 || c >= n + k || used[c]) return PAGAN_E_TREE;
            used[c] = 1;
        }
    for (int v = 0; v < 2 * n - 2; ++v) {
        if (!used[v]) return PAGAN_E_TREE;
        if (!std::isfinite(branch[v]) || branch[v] < 0) return PAGAN_E_TREE;
    }
    return PAGAN_OK;
}

AncSwitches AncSwitches::read() {
    AncSwitches s;
    if (const char *e = std::getenv("PAGAN_ANC_CHUNK_COLS")) s.chunk_cols = std::max(0ll, std::atoll(e));
    return s;
}

int64_t anc_chunk_cols(int32_t n, int64_t columns, int S, int64_t want, const AncSwitches &sw) {
    const int64_t all = std::max<int64_t>(64, (columns + 63) / 64 * 64);
    if (want <= 0) want = sw.chunk_cols;
    if (want <= 0) want = std::max<int64_t>(64, kAncBudgetBytes / (2 * (int64_t)(n - 1) * S * (int64_t)sizeof(double)) / 64 * 64);
    want = want > all ? all : (want + 63) / 64 * 64;               // (compared first: no overflow in the rounding)
    return want;
}

AncLayout::AncLayout(int64_t n, int S, int chars_per_col, int64_t C, int64_t matrices, int64_t n_post) {
    pgdev::Carve c{nullptr};
    const size_t in = (size_t)(n - 1), cols = (size_t)C;
    raw = c.skip((size_t)n * cols * chars_per_col);
    table = c.skip(256 + 64);
    codes = c.skip((size_t)n * cols);
    has = c.skip((size_t)(2 * n - 1) * cols);
    part = c.skip(in * S * cols * sizeof(double));
    outs = c.skip(in * S * cols * sizeof(double));
    P = c.skip((size_t)matrices * S * S * sizeof(double));
    PT = c.skip((size_t)matrices * S * S * sizeof(double));
    pi = c.skip((size_t)S * sizeof(double));
    nodes = c.skip(5 * in * sizeof(int32_t));
    col_lik = c.skip(cols * sizeof(double));
    col_exp = c.skip(cols * sizeof(int32_t));
    best = c.skip(in * cols);
    best_p = c.skip(in * cols * sizeof(float));
    post = c.skip((size_t)n_post * S * cols * sizeof(double));
    total = c.cur;
}

void anc_pmatrix_deriv(const ModelFactory &mf, double t, int order, double *D) {
    const int n = mf.char_as;
    std::fill(D, D + (size_t)n * n, 0.0);
    for (int k = 0; k < n; ++k) {                                  // anc_pmatrix's sum with root[k]^order in every term; no clamp
        const double e1 = (order == 1 ? mf.root[k] : mf.root[k] * mf.root[k]) * std::exp(t * mf.root[k]);
        for (int i = 0; i < n; ++i) {
            const double e2 = mf.U[(size_t)i * n + k] * e1;
            for (int j = 0; j < n; ++j) D[(size_t)i * n + j] += e2 * mf.V[(size_t)k * n + j];
        }
    }
}

AncFitLayout::AncFitLayout(int64_t n, int S, int chars_per_col, int64_t C, int64_t chunks, int64_t matrices) {
    pgdev::Carve c{nullptr};
    const size_t in = (size_t)(n - 1), cols = (size_t)C, nb = (size_t)(2 * n - 2), mat = (size_t)matrices * S * S * sizeof(double);
    raw = c.skip((size_t)n * cols * chars_per_col);
    table = c.skip(256 + 64);
    codes = c.skip((size_t)chunks * n * cols);
    has = c.skip((size_t)chunks * (2 * n - 1) * cols);
    out_has = c.skip((size_t)chunks * (2 * n - 1) * cols);
    part = c.skip(in * S * cols * sizeof(double));
    outs = c.skip(in * S * cols * sizeof(double));
    P = c.skip(mat); PT = c.skip(mat); D1T = c.skip(mat); D2T = c.skip(mat);
    pi = c.skip((size_t)S * sizeof(double));
    nodes = c.skip(5 * in * sizeof(int32_t));
    branches = c.skip(5 * nb * sizeof(int32_t));
    col_lik = c.skip(cols * sizeof(double));
    col_exp = c.skip(cols * sizeof(int32_t));
    best = c.skip(in * cols);
    best_p = c.skip(in * cols * sizeof(float));
    block_sums = c.skip(cols / 64 * nb * 3 * sizeof(double));
    sums = c.skip(nb * 3 * sizeof(double));
    total = c.cur;
}

AncNniLayout::AncNniLayout(int64_t n, int64_t C) {
    pgdev::Carve c{nullptr};
    const size_t in = (size_t)(n - 1), blocks = (size_t)C / 64;
    cand = c.skip((size_t)kNniCandFields * in * sizeof(int32_t));
    block_m = c.skip(blocks * 2 * in * sizeof(double));
    block_e = c.skip(blocks * 4 * in * sizeof(int32_t));
    run_m = c.skip(2 * in * sizeof(double));
    run_e = c.skip(4 * in * sizeof(int64_t));
    total = c.cur;
}

void nni_kinds(int32_t n, const int32_t *left, const int32_t *right, int32_t *kind, int32_t *parent) {
    const int32_t root = 2 * n - 2;
    std::vector<int32_t> par((size_t)2 * n - 1, -1);
    for (int k = 0; k < n - 1; ++k) par[left[k]] = par[right[k]] = n + k;
    for (int k = 0; k < n - 1; ++k) kind[k] = n + k != root && par[n + k] != root ? 1 : 0;
    if (n >= 3 && left[n - 2] >= n && right[n - 2] >= n) kind[left[n - 2] - n] = 2;
    if (parent) std::copy(par.begin(), par.end(), parent);
}

void nni_swap_in_place(int32_t n, std::vector<int32_t> &left, std::vector<int32_t> &right, int32_t node, int32_t k) {
    const int32_t rl = left[n - 2], rr = right[n - 2];
    std::vector<int32_t> &slot = k == 1 ? left : right;            // c's slot that takes b; what it held goes where b was
    if (node == rl && rr >= n) {                                   // the root edge: b = right[rr]
        std::swap(slot[node - n], right[rr - n]);
        return;
    }
    int32_t v = -1;
    for (int q = 0; q < n - 1 && v < 0; ++q) if (left[q] == node || right[q] == node) v = n + q;
    std::vector<int32_t> &sib = left[v - n] == node ? right : left;
    std::swap(slot[node - n], sib[v - n]);
}

void nni_renumber(int32_t n, const std::vector<int32_t> &left, const std::vector<int32_t> &right, const double *branch,
                  int32_t *left_out, int32_t *right_out, double *branch_out, int32_t *perm) {
    std::vector<int32_t> id((size_t)2 * n - 1, -1);
    for (int k = 0; k < n; ++k) id[k] = k;
    int32_t next = n;
    std::vector<std::pair<int32_t, int>> stack{{2 * n - 2, 0}};      // (old id, children visited)
    while (!stack.empty()) {
        auto &[v, stage] = stack.back();
        if (v < n) { stack.pop_back(); continue; }
        if (stage == 0) { stage = 1; stack.push_back({left[v - n], 0}); continue; }
        if (stage == 1) { stage = 2; stack.push_back({right[v - n], 0}); continue; }
        id[v] = next++;
        stack.pop_back();
    }
    for (int k = 0; k < n - 1; ++k) {
        left_out[id[n + k] - n] = id[left[k]];
        right_out[id[n + k] - n] = id[right[k]];
    }
    for (int v = 0; v < 2 * n - 1; ++v) {
        branch_out[id[v]] = branch[v];
        if (perm) perm[v] = id[v];
    }
}

int nni_select(int32_t n, const int32_t *left, const int32_t *right, const double *gain, const int64_t *degenerate, double min_gain,
               int32_t *nodes_out, int32_t *k_out) {
    const int in = n - 1;
    std::vector<int32_t> kind(in), parent((size_t)2 * n - 1);
    nni_kinds(n, left, right, kind.data(), parent.data());
    struct Pick { double gain; int32_t c, k; };
    std::vector<Pick> picks;
    for (int q = 0; q < in; ++q) {
        if (!kind[q]) continue;
        const int k = gain[2 * q + 1] > gain[2 * q] ? 2 : 1;
        const double g = gain[2 * q + k - 1];
        if (degenerate[2 * q + k - 1] == 0 && g > min_gain) picks.push_back({g, n + q, k});
    }
    std::stable_sort(picks.begin(), picks.end(), [](const Pick &x, const Pick &y) { return x.gain > y.gain; });   // (ties: the lower c stays first)
    std::vector<char> taken((size_t)2 * n - 1, 0);
    int count = 0;
    for (const Pick &p : picks) {
        int32_t ends[3] = {p.c, parent[p.c], -1};
        if (kind[p.c - n] == 2) { ends[1] = right[n - 2]; ends[2] = 2 * n - 2; }
        bool free_edge = true;
        for (const int32_t e : ends) if (e >= 0 && taken[e]) free_edge = false;
        if (!free_edge) continue;
        for (const int32_t e : ends) if (e >= 0) taken[e] = 1;
        nodes_out[count] = p.c; k_out[count] = p.k;
        ++count;
    }
    return count;
}

} // namespace pagan

using namespace pagan;

extern "C" {

int pagan_anc_pmatrix(int32_t data_type, const float *base_freq, double t, double *P, double *pi) {
    const int S = anc_states(data_type);
    if (!S || !std::isfinite(t) || t < 0) return PAGAN_E_ARG;
    try {
        ModelFactory mf;
        if (anc_factory(data_type, base_freq, &mf) != PAGAN_OK) return PAGAN_E_INTERNAL;
        if (P) anc_pmatrix(mf, t, P);
        if (pi) std::copy(mf.pi.begin(), mf.pi.begin() + S, pi);
        return S;
    } catch (const std::bad_alloc &) {
        return PAGAN_E_NOMEM;
    }
}

int pagan_anc_rate_matrix(int32_t data_type, const float *base_freq, double *Q, double *pi) {
    const int S = anc_states(data_type);
    if (!S) return PAGAN_E_ARG;
    try {
        ModelFactory mf;
        if (anc_factory(data_type, base_freq, &mf) != PAGAN_OK) return PAGAN_E_INTERNAL;
        if (Q) std::copy(mf.Q.begin(), mf.Q.end(), Q);
        if (pi) std::copy(mf.pi.begin(), mf.pi.begin() + S, pi);
        return S;
    } catch (const std::bad_alloc &) {
        return PAGAN_E_NOMEM;
    }
}

int64_t pagan_anc_encode_row(int32_t data_type, const char *row, uint8_t *codes) {
    if (!anc_states(data_type) || !row) return PAGAN_E_ARG;
    const size_t chars = std::strlen(row), w = data_type == 3 ? 3 : 1;
    if (chars % w) return PAGAN_E_ARG;
    unsigned char table[256], triplet[64];
    anc_leaf_tables(data_type, table, triplet);
    for (size_t c = 0; c < chars / w && codes; ++c) {
        const unsigned char *p = (const unsigned char *)row + c * w;
        if (data_type != 3) { codes[c] = table[p[0]]; continue; }
        const unsigned a = table[p[0]], b = table[p[1]], d = table[p[2]];               // (pa_encode's steps)
        codes[c] = a < 4 && b < 4 && d < 4 ? triplet[a * 16 + b * 4 + d] : kAncMissing;
    }
    return (int64_t)(chars / w);
}

int pagan_anc_check_tree(int32_t n_leaves, const int32_t *left, const int32_t *right, const double *branch) {
    try {
        return anc_check_tree(n_leaves, left, right, branch);
    } catch (const std::bad_alloc &) {
        return PAGAN_E_NOMEM;
    }
}

int64_t pagan_anc_predict_bytes(int32_t n_leaves, int64_t columns, int32_t data_type, int64_t chunk_cols) {
    const int S = anc_states(data_type);
    if (!S || n_leaves < 2 || n_leaves > PAGAN_GUIDE_MAX_SEQS || columns < 0 || columns >= (1ll << 31)) return PAGAN_E_ARG;
    const int64_t C = anc_chunk_cols(n_leaves, columns, S, chunk_cols, AncSwitches::read());
    return (int64_t)AncLayout(n_leaves, S, data_type == 3 ? 3 : 1, C, 2 * (int64_t)n_leaves - 2, n_leaves - 1).total;
}

int pagan_anc_pmatrix_deriv(int32_t data_type, const float *base_freq, double t, int32_t order, double *D) {
    const int S = anc_states(data_type);
    if (!S || !std::isfinite(t) || t < 0 || (order != 1 && order != 2)) return PAGAN_E_ARG;
    try {
        ModelFactory mf;
        if (anc_factory(data_type, base_freq, &mf) != PAGAN_OK) return PAGAN_E_INTERNAL;
        if (D) anc_pmatrix_deriv(mf, t, order, D);
        return S;
    } catch (const std::bad_alloc &) {
        return PAGAN_E_NOMEM;
    }
}

double pagan_anc_branch_step(double t, double g1, double g2, double t_min, double t_max) {
    if (!std::isfinite(t) || !std::isfinite(g1) || !std::isfinite(g2)) return t;
    if (g1 == 0 && g2 == 0) return t;                              // no information
    double s = g2 < 0 ? t - g1 / g2 : g1 > 0 ? 2 * t : t / 2;       // Newton where the curve is concave, else double or halve
    if (s < t / 4) s = t / 4;
    if (s > 4 * t) s = 4 * t;
    if (s < t_min) s = t_min;
    if (s > t_max) s = t_max;
    return s;
}

int64_t pagan_anc_fit_predict_bytes(int32_t n_leaves, int64_t columns, int32_t data_type, int64_t chunk_cols) {
    const int S = anc_states(data_type);
    if (!S || n_leaves < 2 || n_leaves > PAGAN_GUIDE_MAX_SEQS || columns < 0 || columns >= (1ll << 31)) return PAGAN_E_ARG;
    const int64_t C = anc_chunk_cols(n_leaves, columns, S, chunk_cols, AncSwitches::read());
    return (int64_t)AncFitLayout(n_leaves, S, data_type == 3 ? 3 : 1, C, std::max<int64_t>(1, (columns + C - 1) / C), 2 * (int64_t)n_leaves - 2).total;
}

int pagan_anc_nni_apply(int32_t n_leaves, const int32_t *left, const int32_t *right, const double *branch, int32_t node, int32_t k,
                        int32_t *left_out, int32_t *right_out, double *branch_out, int32_t *perm) {
    try {
        const int rc = anc_check_tree(n_leaves, left, right, branch);
        if (rc != PAGAN_OK) return rc;
        const int32_t n = n_leaves;
        if (!left_out || !right_out || !branch_out || node < n || node > 2 * n - 2 || (k != 1 && k != 2)) return PAGAN_E_ARG;
        std::vector<int32_t> kind((size_t)n - 1), l(left, left + n - 1), r(right, right + n - 1);
        nni_kinds(n, left, right, kind.data(), nullptr);
        if (!kind[node - n]) return PAGAN_E_ARG;
        nni_swap_in_place(n, l, r, node, k);
        std::vector<int32_t> lo((size_t)n - 1), ro((size_t)n - 1);   // (the outputs may be the inputs)
        std::vector<double> bo((size_t)2 * n - 1);
        std::vector<int32_t> pm((size_t)2 * n - 1);
        nni_renumber(n, l, r, branch, lo.data(), ro.data(), bo.data(), pm.data());
        bo[(size_t)2 * n - 2] = 0.0;
        std::copy(lo.begin(), lo.end(), left_out); std::copy(ro.begin(), ro.end(), right_out); std::copy(bo.begin(), bo.end(), branch_out);
        if (perm) std::copy(pm.begin(), pm.end(), perm);
        return PAGAN_OK;
    } catch (const std::bad_alloc &) {
        return PAGAN_E_NOMEM;
    }
}

int pagan_anc_nni_select(int32_t n_leaves, const int32_t *left, const int32_t *right, const double *gain, const int64_t *degenerate,
                         double min_gain, int32_t *nodes_out, int32_t *k_out) {
    try {
        if (n_leaves < 2 || !left || !right || !gain || !degenerate || !nodes_out || !k_out || !(min_gain >= 0)) return PAGAN_E_ARG;
        std::vector<double> no_lengths((size_t)2 * n_leaves - 1, 0.0);
        const int rc = anc_check_tree(n_leaves, left, right, no_lengths.data());
        if (rc != PAGAN_OK) return rc;
        return nni_select(n_leaves, left, right, gain, degenerate, min_gain, nodes_out, k_out);
    } catch (const std::bad_alloc &) {
        return PAGAN_E_NOMEM;
    }
}

int64_t pagan_anc_nni_predict_bytes(int32_t n_leaves, int64_t columns, int32_t data_type, int64_t chunk_cols) {
    const int S = anc_states(data_type);
    if (!S || n_leaves < 2 || n_leaves > PAGAN_GUIDE_MAX_SEQS || columns < 0 || columns >= (1ll << 31)) return PAGAN_E_ARG;
    const int64_t C = anc_chunk_cols(n_leaves, columns, S, chunk_cols, AncSwitches::read());
    return (int64_t)(AncFitLayout(n_leaves, S, data_type == 3 ? 3 : 1, C, std::max<int64_t>(1, (columns + C - 1) / C), 2 * (int64_t)n_leaves - 1).total +
                     AncNniLayout(n_leaves, C).total);
}

} // extern "C"
