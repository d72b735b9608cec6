// host_capi.cpp -- the entries of include/pagan_host.h that take no pagan_msa: host graphs on their own, the anchor and tunnel
// helpers, the models and alphabets, the indel fit, the work-queue assignment.
#include <cmath>

#include "host_msa.h"

using namespace pagan;

namespace {

const ModelFactory &codon_factory() {             // the empirical model's eigen solution and 1892 x 1892 tables: made once
    static ModelFactory mf;
    static std::once_flag once;
    std::call_once(once, [] { mf.init_codon(); });
    return mf;
}

} // namespace

extern "C" {

// Work-queue assignment shared by the in-process multi-device walk and the one-process-per-GPU
// bench: units sorted by cost (largest first, stable), each to the currently least-loaded worker.
void pagan_assign_units(int32_t n, const int64_t *cost, int32_t n_workers, int32_t *owner) {
    if (n <= 0 || n_workers <= 0) return;
    std::vector<int> order(n);
    for (int k = 0; k < n; ++k) order[k] = k;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return cost[a] > cost[b]; });
    std::vector<int64_t> load(n_workers, 0);
    for (int k : order) {
        int best = 0;
        for (int d = 1; d < n_workers; ++d) if (load[d] < load[best]) best = d;
        owner[k] = best; load[best] += cost[k];
    }
}

// ---- host graphs on their own -------------------------------------------------------------
pagan_hgraph *pagan_hgraph_leaf(const char *residues, const char *alphabet, int32_t flags) {
    pagan_hgraph *h = new pagan_hgraph();
    h->g = make_leaf(residues, alphabet, flags);
    return h;
}

pagan_hgraph *pagan_hgraph_leaf_codon(const char *nucleotides) {
    if (!nucleotides) return nullptr;
    pagan_hgraph *h = new pagan_hgraph();
    std::string symbols;
    const std::vector<int32_t> states = ModelFactory::codon_states(nucleotides, &symbols);
    h->g = make_leaf_states(states, std::move(symbols), 3, 0);
    return h;
}

pagan_hgraph *pagan_hgraph_parent(pagan_hgraph *l, pagan_hgraph *r, const pagan_result *res, float lbl, float rbl,
                                  const int32_t *parsimony, int32_t S, int32_t char_as, int32_t flags) {
    BuildSettings bs;
    if (flags & 1) bs.reads_mode();
    if (flags & 2) bs.reduced_terminal = false;
    pagan_hgraph *h = new pagan_hgraph();
    h->g = make_parent(l->g, r->g, *res, lbl, rbl, parsimony, S, char_as, bs);
    return h;
}

// The same graph built on the current device (dp_parent.hip).  NULL without a device or on a HIP error -- never a host-built
// graph in its place.  info (may be NULL): runs of skipped sites, fixpoint rounds of the boundary pass, deleted sites, edge
// weights outside the log table, log weights the host had to put right.
pagan_hgraph *pagan_hgraph_parent_device(pagan_hgraph *l, pagan_hgraph *r, const pagan_result *res, float lbl, float rbl,
                                         const int32_t *parsimony, int32_t S, int32_t char_as, int32_t flags, int32_t *info) {
    BuildSettings bs;
    if (flags & 1) bs.reads_mode();
    if (flags & 2) bs.reduced_terminal = false;
    pagan_hgraph *h = new pagan_hgraph();
    ParentBuildInfo pi;
    if (!make_parent_device(l->g, r->g, *res, lbl, rbl, parsimony, S, char_as, bs, -1, &h->g, &pi)) { delete h; return nullptr; }
    if (info) { info[0] = pi.runs; info[1] = pi.rounds; info[2] = pi.deleted_sites; info[3] = pi.weights_outside_table; info[4] = pi.log_weights_patched; }
    return h;
}

void pagan_hgraph_view(const pagan_hgraph *g, pagan_graph *out) { *out = g->g.view(); }

void pagan_hgraph_attrs(const pagan_hgraph *h, int32_t *sa, float *sd, int32_t *ea, float *ef) {
    const SeqGraph &g = h->g;
    std::vector<char> linked(g.n_edges(), 0);
    for (int e : g.fwd_eid) linked[e] = 1;
    for (int s = 0; s < g.n_sites(); ++s) {
        int32_t *a = sa + 8 * s;
        a[0] = g.state[s]; a[1] = g.site_type[s]; a[2] = g.path_state[s]; a[3] = g.child_l[s]; a[4] = g.child_r[s];
        a[5] = g.count_since_used[s]; a[6] = g.ambiguous[s]; a[7] = g.fwd_off[s + 1] - g.fwd_off[s];
        sd[s] = g.dist_since_used[s];
    }
    for (int e = 0; e < g.n_edges(); ++e) {
        int32_t *a = ea + 6 * e;
        a[0] = g.e_start[e]; a[1] = g.e_end[e]; a[2] = g.e_used[e]; a[3] = g.e_count_since_used[e];
        a[4] = g.e_count_as_skipped[e]; a[5] = linked[e];
        ef[3 * e] = g.e_w[e]; ef[3 * e + 1] = g.e_logw[e]; ef[3 * e + 2] = g.e_dist_since_used[e];
    }
}

void pagan_hgraph_fwd(const pagan_hgraph *h, int32_t *fwd_off, int32_t *fwd_eid) {
    std::memcpy(fwd_off, h->g.fwd_off.data(), sizeof(int32_t) * h->g.fwd_off.size());
    if (!h->g.fwd_eid.empty()) std::memcpy(fwd_eid, h->g.fwd_eid.data(), sizeof(int32_t) * h->g.fwd_eid.size());
}

int pagan_hgraph_string(const pagan_hgraph *h, int32_t with_gaps, const char *alphabet, char *out) {
    const std::string s = sequence_string(h->g, with_gaps != 0, alphabet);
    std::memcpy(out, s.c_str(), s.size() + 1);
    return (int)s.size();
}

void pagan_hgraph_free(pagan_hgraph *g) { delete g; }

int pagan_define_tunnel(const char *s1, const char *s2, const char *g1, const char *g2, int32_t prefix_hit_length,
                        int32_t hit_trim, int32_t offset, int32_t *upper, int32_t *lower) {
    AnchorSettings as;
    as.prefix_hit_length = prefix_hit_length; as.hit_trim = hit_trim; as.offset = offset;
    std::vector<int32_t> up, lo;
    const int n = define_tunnel(s1, s2, g1, g2, as, &up, &lo);
    std::memcpy(upper, up.data(), sizeof(int32_t) * up.size());
    std::memcpy(lower, lo.data(), sizeof(int32_t) * lo.size());
    return n;
}

int pagan_prefix_hits(const char *s1, const char *s2, int32_t min_length, int32_t *hits, int32_t cap) {
    if (!s1 || !s2) return PAGAN_E_ARG;
    std::vector<Hit> v;
    prefix_hits(s1, s2, min_length, &v);
    for (size_t k = 0; k < v.size() && (int)k < cap; ++k) { hits[4 * k] = v[k].s1; hits[4 * k + 1] = v[k].s2; hits[4 * k + 2] = v[k].len; hits[4 * k + 3] = v[k].score; }
    return (int)v.size();
}

int pagan_prefix_hits_raw(const char *s1, const char *s2, int32_t min_length, int32_t where, int32_t *hits, int32_t cap) {
    if (!s1 || !s2 || min_length < 1 || cap < 0 || (cap > 0 && !hits) || (where != 0 && where != 1)) return PAGAN_E_ARG;
    std::vector<Hit> v;
    if (where == 0) prefix_hits_raw_host(s1, s2, min_length, &v);
    else if (!prefix_hits_device(s1, s2, min_length, &v, anchor_device())) return PAGAN_E_NODEVICE;
    for (size_t k = 0; k < v.size() && (int)k < cap; ++k) { hits[3 * k] = v[k].s1; hits[3 * k + 1] = v[k].s2; hits[3 * k + 2] = v[k].len; }
    return (int)v.size();
}

long long pagan_anchors_device_calls(void) { return device_finder_calls.load(); }

int pagan_drop_bad_hits(int32_t *hits, int32_t n, int32_t thr_total, int32_t thr_partly) {
    if (n < 0 || (n > 0 && !hits)) return PAGAN_E_ARG;
    std::vector<Hit> v(n);
    for (int k = 0; k < n; ++k) v[k] = Hit{hits[4 * k], hits[4 * k + 1], hits[4 * k + 2], hits[4 * k + 3]};
    drop_bad_hits(&v, (unsigned)thr_total, (unsigned)thr_partly);
    for (size_t k = 0; k < v.size(); ++k) { hits[4 * k] = v[k].s1; hits[4 * k + 1] = v[k].s2; hits[4 * k + 2] = v[k].len; hits[4 * k + 3] = v[k].score; }
    return (int)v.size();
}

int pagan_define_tunnel_overlapping(const int32_t *hits, int32_t n, const char *g1, const char *g2, int32_t width,
                                    int32_t *upper, int32_t *lower, int32_t *blocks, int32_t cap) {
    if (n < 0 || (n > 0 && !hits) || !g1 || !g2 || !upper || !lower) return PAGAN_E_ARG;
    std::vector<Hit> v(n);
    for (int k = 0; k < n; ++k) v[k] = Hit{hits[4 * k], hits[4 * k + 1], hits[4 * k + 2], hits[4 * k + 3]};
    std::vector<int32_t> up, lo;
    std::vector<TunnelBlock> eb;
    hits_to_band_overlapping(v, g1, g2, width, &up, &lo, &eb);
    std::memcpy(upper, up.data(), sizeof(int32_t) * up.size());
    std::memcpy(lower, lo.data(), sizeof(int32_t) * lo.size());
    for (size_t k = 0; k < eb.size() && (int)k < cap; ++k) { blocks[4 * k] = eb[k].sx; blocks[4 * k + 1] = eb[k].sy; blocks[4 * k + 2] = eb[k].ex; blocks[4 * k + 3] = eb[k].ey; }
    return (int)eb.size();
}

int pagan_force_gap(int32_t *upper, int32_t *lower, int32_t n, const int32_t *blocks, int32_t n_blocks, int32_t threshold,
                    int32_t width, int32_t wide) {
    if (!upper || !lower || n < 1 || n_blocks < 0 || (n_blocks > 0 && !blocks)) return PAGAN_E_ARG;
    std::vector<int32_t> up(upper, upper + n), lo(lower, lower + n);
    std::vector<TunnelBlock> eb(n_blocks);
    for (int k = 0; k < n_blocks; ++k) { eb[k].sx = blocks[4 * k]; eb[k].sy = blocks[4 * k + 1]; eb[k].ex = blocks[4 * k + 2]; eb[k].ey = blocks[4 * k + 3]; }
    const bool done = force_gap(&up, &lo, &eb, threshold, width, wide != 0);
    std::memcpy(upper, up.data(), sizeof(int32_t) * n);
    std::memcpy(lower, lo.data(), sizeof(int32_t) * n);
    return done ? 1 : 0;
}

int pagan_dna_model(const float bf[4], double distance, float *table, float *params, int32_t *parsimony) {
    if (!bf || !table || !params) return PAGAN_E_ARG;
    ModelFactory mf;
    mf.init_dna(bf);
    const EvolModel em = mf.alignment_model(distance);
    std::memcpy(table, em.log_score.data(), sizeof(float) * 225);
    params[0] = em.log_gap_open; params[1] = em.log_gap_ext; params[2] = em.log_gap_end_ext; params[3] = em.log_non_gap;
    if (parsimony) std::memcpy(parsimony, mf.parsimony.data(), sizeof(int32_t) * 225);
    return PAGAN_OK;
}

int pagan_protein_model(double distance, float *table, float *params, int32_t *parsimony) {
    if (!table || !params) return PAGAN_E_ARG;
    static ModelFactory mf;                       // the WAG eigen solution does not depend on the input
    static std::once_flag once;
    std::call_once(once, [] { mf.init_protein(); });
    const EvolModel em = mf.alignment_model(distance);
    std::memcpy(table, em.log_score.data(), sizeof(float) * em.log_score.size());
    params[0] = em.log_gap_open; params[1] = em.log_gap_ext; params[2] = em.log_gap_end_ext; params[3] = em.log_non_gap;
    if (parsimony) std::memcpy(parsimony, mf.parsimony.data(), sizeof(int32_t) * mf.parsimony.size());
    return PAGAN_OK;
}

int pagan_codon_model(double distance, float *table, float *params, int32_t *parsimony) {
    if (!table || !params) return PAGAN_E_ARG;
    const ModelFactory &mf = codon_factory();
    const EvolModel em = mf.alignment_model(distance);
    std::memcpy(table, em.log_score.data(), sizeof(float) * em.log_score.size());
    params[0] = em.log_gap_open; params[1] = em.log_gap_ext; params[2] = em.log_gap_end_ext; params[3] = em.log_non_gap;
    if (parsimony) std::memcpy(parsimony, mf.parsimony.data(), sizeof(int32_t) * mf.parsimony.size());
    return PAGAN_OK;
}

int pagan_codon_alphabet(char *names, int32_t *mostcommon) {
    const ModelFactory &mf = codon_factory();
    if (names) std::memcpy(names, mf.codon_names.c_str(), mf.codon_names.size() + 1);
    if (mostcommon) std::memcpy(mostcommon, mf.mostcommon.data(), sizeof(int32_t) * mf.mostcommon.size());
    return mf.S;
}

int pagan_codon_translate(const char *codons, char *out) {
    if (!codons || !out) return PAGAN_E_ARG;
    const std::string p = ModelFactory::translate_codons(codons);
    std::memcpy(out, p.c_str(), p.size() + 1);
    return (int)p.size();
}

int pagan_codon_states(const char *nucleotides, int32_t *states) {
    if (!nucleotides || !states) return PAGAN_E_ARG;
    const std::vector<int32_t> st = ModelFactory::codon_states(nucleotides);
    if (!st.empty()) std::memcpy(states, st.data(), sizeof(int32_t) * st.size());
    return (int)st.size();
}

// Probability-space view of the same model (Evol_model::score / gap_open / gap_ext / non_gap): score [a + b*S],
// params[3] = gap_open, gap_ext, non_gap.  data_type 1: DNA (base_freq needed), 2: protein, 3: codon.
int pagan_model_prob_table(int32_t data_type, const float *base_freq, double distance, float *score, float *params) {
    if (!score || !params || (data_type != 2 && data_type != 3 && !base_freq)) return PAGAN_E_ARG;
    ModelFactory own;
    if (data_type == 2) own.init_protein(); else if (data_type != 3) own.init_dna(base_freq);
    const ModelFactory &mf = data_type == 3 ? codon_factory() : own;
    const EvolModel em = mf.alignment_model(distance);
    std::memcpy(score, em.score.data(), sizeof(float) * em.score.size());
    params[0] = em.gap_open; params[1] = em.gap_ext; params[2] = em.non_gap;
    return PAGAN_OK;
}

int pagan_model_alphabets(int32_t data_type, char *leaf_alphabet, char *ancestral_alphabet) {
    ModelFactory mf;
    if (data_type == 2) mf.init_protein();
    else { const float bf[4] = {0.25f, 0.25f, 0.25f, 0.25f}; mf.init_dna(bf); }
    if (leaf_alphabet) std::memcpy(leaf_alphabet, mf.leaf_alphabet.c_str(), mf.leaf_alphabet.size() + 1);
    if (ancestral_alphabet) std::memcpy(ancestral_alphabet, mf.ancestral_alphabet.c_str(), mf.ancestral_alphabet.size() + 1);
    return mf.S;
}

int pagan_eigen_qrev(const double *Q, const double *pi, int32_t n, double *root, double *U, double *V) {
    if (!Q || !pi || n < 1 || !root || !U || !V) return PAGAN_E_ARG;
    return eigen_qrev(Q, pi, n, root, U, V);
}

// A moment / pseudo-likelihood estimate of the indel model from the nodes' expected counts (include/pagan_host.h).
int pagan_fit_indel(int32_t n, const double *dist, const double *trans, double *indel_rate, double *gap_ext) {
    if (n < 0 || (n > 0 && (!dist || !trans)) || !indel_rate || !gap_ext) return PAGAN_E_ARG;
    double stay = 0, leave = 0, d_max = 0;
    std::vector<double> O(n), Sm(n);
    bool any_open = false, any = false;
    for (int k = 0; k < n; ++k) {
        const double *t = trans + 12 * (size_t)k;
        for (int q = 0; q < 12; ++q) if (!(t[q] >= 0.0) || !(t[q] < HUGE_VAL)) return PAGAN_E_ARG;
        if (!(dist[k] >= 0.0) || !(dist[k] < HUGE_VAL)) return PAGAN_E_ARG;
        stay += t[0] + t[4];                                        // n_XX + n_YY
        leave += t[1] + t[3] + t[2] + t[5] + t[9] + t[10];          // n_XY + n_YX + n_XM + n_YM + n_Xend + n_Yend
        O[k] = t[6] + t[7]; Sm[k] = t[8] + t[11];                   // n_MX + n_MY; n_MM + n_Mend
        if (dist[k] > 0 && O[k] + Sm[k] > 0) { any = true; any_open = any_open || O[k] > 0; d_max = std::max(d_max, dist[k]); }
    }
    *gap_ext = stay + leave > 0 ? stay / (stay + leave) : 0.0;
    *indel_rate = 0.0;
    if (!any || !any_open) return PAGAN_OK;                         // (no transition out of a match seen, or no gap opened: rate 0)
    // g(r) = sum_k d_k [ O_k (1 - t_k) / (2 t_k) - S_k (1 - t_k) / (1 - 2 t_k) ], t_k = 1 - exp(-0.5 r d_k): the derivative of the
    // objective by r; it falls from +inf at r = 0 and reaches -inf where 1 - 2 t_k = 0 at the longest distance (r d_max = 2 ln 2),
    // unless no node with d = d_max has S > 0, when the root may lie at the bound itself
    auto g = [&](double r) {
        double s = 0;
        for (int k = 0; k < n; ++k) {
            if (!(dist[k] > 0) || !(O[k] + Sm[k] > 0)) continue;
            const double e = std::exp(-0.5 * r * dist[k]), tk = 1.0 - e;
            s += dist[k] * (O[k] * e / (2 * tk) - Sm[k] * e / (1.0 - 2 * tk));
        }
        return s;
    };
    double lo = 0.0, hi = 2.0 * std::log(2.0) / d_max;
    for (int it = 0; it < 200 && hi - lo > 1e-13 * hi; ++it) {
        const double mid = 0.5 * (lo + hi);
        const double v = g(mid);
        if (v > 0) lo = mid; else hi = mid;                         // (NaN at the bound itself -- inf - inf -- counts as beyond the root)
    }
    *indel_rate = 0.25 * (lo + hi);                                 // r / 2
    return PAGAN_OK;
}

} // extern "C"
