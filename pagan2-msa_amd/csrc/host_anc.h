// host_anc.h -- what dp_anc.hip (pruning and the outside pass on the device) takes from host_anc.cpp (the transition matrices,
// the leaf tables, the tree check, the chunk size and the device layout).  The definitions are in include/pagan_host.h,
// "ancestral states by marginal likelihood".
#ifndef PAGAN_HOST_ANC_H
#define PAGAN_HOST_ANC_H

#include <cstddef>
#include <cstdint>
#include <vector>

#include "host_model.h"

namespace pagan {

constexpr unsigned char kAncMissing = 0xFF;      // protein, codon: no state.  DNA codes are state sets (bit s: state s), 0 is missing.
constexpr int64_t kAncBudgetBytes = 1ll << 30;   // what the default chunk size keeps the partials and outside vectors under

// S of data_type 1 / 2 / 3, 0 for anything else
int anc_states(int data_type);
// the factory of data_type 1 / 2 / 3 (DNA: base_freq, null = 0.25 each, kappa and rho at the walk's defaults) with Q, U, V, root those
// of the rate matrix made proper (host_anc.cpp).  PAGAN_OK, or PAGAN_E_INTERNAL where the eigen solver failed.
int anc_factory(int data_type, const float *base_freq, ModelFactory *mf);
// P [S * S] row-major for length t by Eigen::computePMatrix's sum as alignment_model restates it, clamped at 0; t == 0: identity
void anc_pmatrix(const ModelFactory &mf, double t, double *P);
// DNA: table[c] the state set of character c (0: missing).  Protein: table[c] the state or kAncMissing.  Codon: table[c] the base
// 0..3 or kAncMissing, and triplet[16 a + 4 b + c] the state of the codon or kAncMissing (stop codons).
void anc_leaf_tables(int data_type, unsigned char table[256], unsigned char triplet[64]);
int anc_check_tree(int32_t n, const int32_t *left, const int32_t *right, const double *branch);

// the switches of the environment, read once a call
struct AncSwitches {
    int64_t chunk_cols = 0;          // PAGAN_ANC_CHUNK_COLS: > 0 forces the columns of a chunk (rounded up to 64)
    static AncSwitches read();
};
// the columns of a chunk: `want` (<= 0: the switch, else what kAncBudgetBytes holds) rounded up to 64, at most `columns` rounded up to 64
int64_t anc_chunk_cols(int32_t n, int64_t columns, int S, int64_t want, const AncSwitches &sw);

// the device buffers of one pagan_anc_reconstruct call, carved from one allocation; C = columns of a chunk (a multiple of 64)
struct AncLayout {
    size_t raw, table, codes, has, part, outs, P, PT, pi, nodes, col_lik, col_exp, best, best_p, post, total;
    AncLayout(int64_t n, int S, int chars_per_col, int64_t C, int64_t matrices, int64_t n_post);
};

// ---- branch lengths by maximum likelihood (include/pagan_host.h, "branch lengths by maximum likelihood") ----------------
// D_order(t) [S * S] row-major, order 1 or 2: anc_pmatrix's sum with root[k]^order in every term, not clamped
void anc_pmatrix_deriv(const ModelFactory &mf, double t, int order, double *D);

// the device buffers of one fit or derivative call; the codes, has_data and out_has of all `chunks` chunks stay resident, the
// rest is one chunk's
struct AncFitLayout {
    size_t raw, table, codes, has, out_has, part, outs, P, PT, D1T, D2T, pi, nodes, branches, col_lik, col_exp, best, best_p, block_sums, sums, total;
    AncFitLayout(int64_t n, int S, int chars_per_col, int64_t C, int64_t chunks, int64_t matrices);
};

// ---- tree search by nearest-neighbour interchange (include/pagan_host.h, "tree search by nearest-neighbour interchange") ----
constexpr int kNniCandFields = 11;   // the candidate table's rows: a, d, b, e (-1: ordinary), the matrices of a, d, b, e, P_mid's,
                                     // the parent's index among the internal nodes (-1: the root edge), the node c itself

// what a search keeps beside the fit's buffers (AncFitLayout with one matrix more, for the root edge's P_mid), in an allocation
// of its own.  in = n - 1 slots for the candidates, whatever the tree.
struct AncNniLayout {
    size_t cand, block_m, block_e, run_m, run_e, total;    // [11][in] int32, [C/64][2][in] fp64, [C/64][4][in] int32, [2][in] fp64, [4][in] int64
    AncNniLayout(int64_t n, int64_t C);
};

// kind [n-1] by internal node: 0 no candidate, 1 ordinary, 2 the root edge (at left[root]); parent [2n-1] (the root's -1) may be null
void nni_kinds(int32_t n, const int32_t *left, const int32_t *right, int32_t *kind, int32_t *parent);
// one swap in place, on ids that stay (no renumbering); node and k are taken as valid
void nni_swap_in_place(int32_t n, std::vector<int32_t> &left, std::vector<int32_t> &right, int32_t node, int32_t k);
// the internal nodes renumbered in post-order (left subtree, right subtree, the node); perm [2n-1]: the new id of every old one
void nni_renumber(int32_t n, const std::vector<int32_t> &left, const std::vector<int32_t> &right, const double *branch,
                  int32_t *left_out, int32_t *right_out, double *branch_out, int32_t *perm);
// the selection; nodes_out, k_out [n-1]; returns how many
int nni_select(int32_t n, const int32_t *left, const int32_t *right, const double *gain, const int64_t *degenerate, double min_gain,
               int32_t *nodes_out, int32_t *k_out);

} // namespace pagan

#endif
