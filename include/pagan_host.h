/*
 * pagan_host.h -- C ABI of the host-side guide-tree walk that drives pagan_dp.h.
 *
 * Mirrors the part of the reference's Node class that calls the aligner:
 * Node::start_alignment / start_openmp_alignment -> align_sequences_this_node
 * (src/main/node.h:880-938, src/main/node.cpp:52-285): post-order over a rooted binary guide
 * tree; at every internal node build the Evol_model for dist = d_left + d_right, define the
 * tunnel from anchors, call the pairwise aligner (GPU), build the parent Sequence graph.
 * Nodes whose children are finished are independent and are aligned as one batch
 * (node.cpp:227-285), optionally spread over several devices or ranks (no collectives in the
 * data path: what ranks exchange is the finished path of a node, host bytes).
 *
 * Also exposes the host graph builder on its own (pagan_hgraph_*), the counterpart of
 * Sequence construction (src/main/sequence.cpp:152-303) and
 * Basic_alignment::build_ancestral_sequence (src/main/basic_alignment.cpp:36-653).
 */
#ifndef PAGAN_HOST_H
#define PAGAN_HOST_H

#include <stdint.h>
#include "pagan_dp.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PAGAN_E_TREE   -20   /* Newick parse error / tree not rooted binary / unknown leaf */
#define PAGAN_E_MEMCAP -21   /* one alignment would not fit the device memory budget         */

typedef struct pagan_msa pagan_msa;

typedef struct pagan_msa_opts {
    int32_t  use_anchors;        /* 0 = --no-anchors (full matrix), 1 = --use-prefix-anchors      */
    int32_t  anchors_offset;     /* --anchors-offset, default 15 (settings.cpp:157)              */
    int32_t  prefix_hit_length;  /* --prefix-hit-length, default 30 (settings.cpp:160)           */
    int32_t  hit_trim;           /* --exonerate-hit-trim, default 5 (settings.cpp:155)           */
    uint32_t dp_flags;           /* PAGAN_OPT_*                                                  */
    int32_t  leaf_flags;         /* 1 = --454, 2 = --homopolymer (sequence.cpp:205,253)          */
    int32_t  keep_all_edges;     /* --keep-all-edges (basic_alignment.h:572-586)                 */
    int32_t  n_devices;          /* devices to farm ready nodes over; 0 = just the current one   */
    int32_t  first_device;       /* ordinal of the first device used                             */
    int32_t  host_threads;       /* threads for anchors / graph building; 0 = hardware           */
    float    truncate_branches;  /* --truncate-branches, default 0.2 (settings.cpp:228)          */
    int64_t  device_mem_budget;  /* bytes of HBM one batch may use; 0 = 80% of free memory       */
    int32_t  data_type;          /* 0 = guess (Fasta_reader::check_sequence_data_type,
                                    fasta_reader.cpp:1303-1336), 1 = DNA, 2 = protein (WAG,
                                    211-letter alphabet, model_factory.cpp:304-632,1478-1595),
                                    3 = DNA read as codons (--codons: 1892 states, rows of three
                                    characters per column; anchors are found in the codon
                                    strings' translation, viterbi_alignment.cpp:54-60)            */
    int32_t  pileup_rates;       /* ins = del = 0.25: --454/--homopolymer with --pileup-alignment
                                    (model_factory.cpp:1901-1905)                                  */
    int32_t  anchor_mode;        /* 0 = order-conflict filter + Find_anchors::define_tunnel
                                    (viterbi_alignment.cpp:159-164); 1 = eliminate_bad_hits +
                                    define_tunnel_with_overlapping_hits (:148-157, the BLAST branch;
                                    the hits here are the prefix anchors)                          */
    int32_t  overlap_total;      /* --ncbi-threshold-overlap-total, default 50 (settings.cpp:180)  */
    int32_t  overlap_partly;     /* --ncbi-threshold-overlap-partly, default 400 (settings.cpp:181) */
    int32_t  force_gap;          /* --force-gap (node.cpp:124-141): over the memory budget, replace the
                                    largest empty tunnel block by a gap until the node fits         */
    int32_t  force_gap_threshold;/* --force-gap-threshold, default 40000 (settings.cpp:189)        */
    int32_t  force_gap_wide;     /* --force-gap-wide-tunnel                                        */
    int32_t  mostcommon;         /* --mostcommon: a matched column's parent state from the most-common table
                                    (basic_alignment.cpp:146-147) and Node::fix_ambiguous_states
                                    (node.cpp:1610-1690) after every node                            */
    int32_t  full_probability;   /* --full-probability (viterbi_alignment.cpp:329-371): 1 = behind every node's Viterbi
                                    alignment, on the band the node finally used, the forward/backward pass runs on the GPU
                                    (pagan_fb_run_batch, the model's probability-space view at the node's distance) and the
                                    node keeps log_fwd, log_bwd and the posterior support of its path's columns; 2 = its
                                    site marginals too.  The alignment itself does not change.                         */
    int32_t  sample_path;        /* --sample-path (viterbi_alignment.cpp:395-417): 1 = no Viterbi alignment; every node's
                                    path is sampled from its forward matrix (pagan_fb_sample_path, on the host: the
                                    forward matrix is downloaded, 24 B a cell) with pagan_sample_uniforms(sample_seed,
                                    public node id, Lx + Ly + 1); node score = log full probability; a tunnel whose full
                                    probability is 0 is retried without the tunnel                                      */
    uint64_t sample_seed;
} pagan_msa_opts;

void pagan_msa_default_opts(pagan_msa_opts *o);

/* The work-queue rule that spreads a tree level's ready nodes (node.cpp:273-285 run_nodes) over
 * devices or ranks: largest cost first, each unit to the least-loaded worker.  owner[k] in
 * [0, n_workers).  Pure host function (no GPU).                                             */
void pagan_assign_units(int32_t n, const int64_t *cost, int32_t n_workers, int32_t *owner);

typedef struct pagan_node_info {
    int32_t node, left, right;   /* node ids: leaves 0..n-1 in input order, internal n..2n-2
                                    in alignment (post-order) order                              */
    int32_t level;               /* batch (tree level) the node was aligned in                   */
    int32_t left_sites, right_sites, sites;
    int32_t n_hits;
    int64_t cells;
    double  dist;                /* d_left + d_right after truncation (node.cpp:70)               */
    double  score;
    int32_t status;
    int32_t n_forced_gaps;       /* empty tunnel blocks replaced by a gap (--force-gap)             */
} pagan_node_info;

typedef struct pagan_msa_timing {
    double total_s, model_s, anchors_s, dp_wall_s, dp_fill_dev_s, dp_trace_dev_s, build_s;
} pagan_msa_timing;

int  pagan_msa_create(int32_t n_seqs, const char *const *names, const char *const *seqs,
                      const char *newick, const pagan_msa_opts *opts, pagan_msa **out);
/* Progressive alignment of every internal node; the DP runs on the GPU(s).  With n_devices > 1 the
 * ready nodes are a work queue over the devices (Node::start_threaded_alignment, node.cpp:196-223,
 * 289-345): a parent is ready the moment its two children are done, idle devices take what is
 * ready.  No collective: parents are built on the host.                                          */
int  pagan_msa_align(pagan_msa *m);

/* ---- the same walk, one step at a time (one process per GPU: tree replicated, DP sharded) -------
 * Every rank holds the whole tree.  Per round: pagan_msa_ready lists the nodes whose children are
 * done (build_queues, node.cpp:273-285; the same list on every rank), the ranks split it with
 * pagan_assign_units over pagan_msa_node_cost, each aligns its share (pagan_msa_align_nodes:
 * model, anchors, DP on this rank's device(s), parent graph), exports what the alignment left behind
 * (pagan_msa_export_result: path columns + used child edges + max_end, a few bytes per column) and
 * imports the other ranks' results (pagan_msa_import_result stores them; the parent graph of an
 * imported node is built when this process needs it -- when it claims a node above, or is asked for
 * the rows -- so the ranks shard the parent graphs as they shard the alignments: node.cpp:196-223,
 * 273-345, a thread builds the ancestor of the node it aligned).  pagan_msa_finish after the last
 * round builds what is pending and the rows; pagan_msa_finish_lazy leaves both to the first call
 * that needs them (a rank that is never asked for the alignment never builds them).
 * pagan_msa_align is this loop with one rank.                                                  */
int     pagan_msa_ready(const pagan_msa *m, int32_t *ids, int32_t cap);    /* count (may exceed cap) */
int     pagan_msa_remaining(const pagan_msa *m);                           /* internal nodes not yet done */
int64_t pagan_msa_node_cost(const pagan_msa *m, int32_t node);             /* cells estimate of a ready node */
int     pagan_msa_align_nodes(pagan_msa *m, int32_t n, const int32_t *nodes);
int64_t pagan_msa_export_result(const pagan_msa *m, int32_t node, void *buf, int64_t cap);  /* bytes needed/written */
int     pagan_msa_import_result(pagan_msa *m, const void *buf, int64_t bytes);
int     pagan_msa_finish(pagan_msa *m);
int     pagan_msa_finish_lazy(pagan_msa *m);
int     pagan_msa_parents_built(const pagan_msa *m);                       /* parent graphs this process has built so far */
int     pagan_msa_data_type(const pagan_msa *m);                           /* 1 DNA, 2 protein */
int     pagan_msa_node_device(const pagan_msa *m, int32_t k);              /* device internal node k ran on; -1: another rank */
/* TEST SEAM, never set by the product: replaces pagan_dp_align_batch as the thing the work queue hands its
 * batches to, so that the queue (dealing, feeder threads, retries, result exchange) can be exercised on a
 * machine without a GPU (with full_probability or sample_path set the walk then fails with PAGAN_E_NODEVICE: the seam has
 * no forward/backward pass, and the pass is never skipped silently).  fn has pagan_dp_align_batch's contract (results released with free()); the device a
 * batch was dealt to arrives in opts->device.  NULL restores the HIP path.                                    */
typedef int (*pagan_batch_fn)(int32_t n, const pagan_job *jobs, const pagan_opts *opts, pagan_result *out, void *user);
int     pagan_msa_set_batch_backend(pagan_msa *m, pagan_batch_fn fn, void *user);
/* Where a walk with sample_path set draws its paths (a setter: pagan_msa_opts does not grow).  0, the default: on the host,
 * pagan_fb_sample_path behind a download of the node's forward matrix (24 B a cell).  1: on the device -- a sub-batch's nodes
 * go through one pagan_fb_sample_paths_batch(n, fbs, sample_seed, public node ids, 1, 0), a node's result is the replay of
 * its path 0, and 12 B a path step come to the host.  The same paths either way (pagan_dp.h); support, the retry without the
 * tunnel and the totals do not change; the sampler's device time is added to pagan_msa_node_fb's out[3] at the sub-batch's
 * first node.  Call before aligning.                                                                                        */
int     pagan_msa_set_sampler(pagan_msa *m, int32_t on_device);
/* Posterior decoding in the walk (a setter: pagan_msa_opts does not grow).  on = 1: there is no Viterbi batch, as under
 * sample_path; a unit's nodes go through pagan_fb_run_batch in sub-batches cut by pagan_fb_predict_bytes_states +
 * pagan_fb_decode_predict_bytes, each sub-batch through one pagan_fb_decode_batch(n, fbs, gap_weight, 0), and a node's result is
 * the replay of its maximum expected accuracy path (pagan_dp.h): score = log full probability, support along the decoded path,
 * a band whose full probability is 0 retried without the band.  Together with sample_path: PAGAN_E_ARG at align time; with the
 * test seam: PAGAN_E_NODEVICE.  gap_weight: a finite double >= 0 (0.5: a residue counts once).  Call before aligning.           */
int     pagan_msa_set_decoder(pagan_msa *m, int32_t on, double gap_weight);
/* Expected counts in the walk (a setter: pagan_msa_opts does not grow).  on = 1: wherever a node's forward/backward pass runs
 * (full_probability, sample_path, the decoder) the node also keeps pagan_fb_expected_counts' trans[12] and, for DNA, emit[S * S]
 * (pagan_dp.h); a sub-batch's counts are taken in one pagan_fb_expected_counts_batch before its matrices are released, and the
 * device time is added to pagan_msa_node_fb's out[3] at the sub-batch's first node.  Without any such pass: PAGAN_E_ARG at align
 * time.  Nothing else of the walk changes.  Call before aligning.                                                              */
int     pagan_msa_set_counts(pagan_msa *m, int32_t on);
/* node_counts (pagan_msa_set_counts): trans[12]; emit[S * S] or NULL (protein and codon walks keep no table: emit non-NULL is
 * PAGAN_E_ARG there).  PAGAN_E_ARG for a node this process did not align, as for the support.                                 */
int     pagan_msa_node_counts(const pagan_msa *m, int32_t k, double *trans, double *emit);
/* The indel model of the walk, the reference's --ins-rate, --del-rate, --gap-extension, --end-gap-extension (settings.cpp:216-218,
 * 266-267): the values replace the data type's defaults (DNA 0.01 / 0.01 / 0.8 / 0.95, protein 0.05 / 0.05 / 0.5 / 0.75, codon
 * 0.01 / 0.01 / 0.5 / 0.75) in both model views -- gap_open = t = 1 - exp(-0.5 (ins + del) dist), non_gap = 1 - 2 t at a node's
 * distance --; a negative value keeps the default; pileup_rates still replaces the two rates where it applies.  gap_ext and
 * end_gap_ext are probabilities in (0, 1).  Call before aligning (after: PAGAN_E_ARG).  Rates that give 1 - 2 t <= 0 at some
 * internal node's distance: PAGAN_E_ARG at align time.                                                                         */
int     pagan_msa_set_indel_model(pagan_msa *m, double ins_rate, double del_rate, double gap_ext, double end_gap_ext);
/* Host only, plain arithmetic: an indel rate and a gap extension probability from n nodes' distances dist[n] (the sum of the two
 * child branches) and expected counts trans[n][12] -- "align, count, refit, realign".
 *   gap_ext    = (n_XX + n_YY) / (n_XX + n_YY + n_XY + n_YX + n_XM + n_YM + n_Xend + n_Yend): the share of the steps out of a gap
 *                cell that stay in the gap; 0 when no step out of a gap cell was counted.
 *   indel_rate = r / 2, r = ins + del the maximiser of sum_k O_k log t_k + S_k log(1 - 2 t_k), t_k = 1 - exp(-0.5 r d_k),
 *                O_k = n_MX + n_MY, S_k = n_MM + n_Mend, found by bisection on the derivative over 0 < r d_max < 2 ln 2 to
 *                1e-13 relative (one node: t = O / (2 (O + S))); 0 when no node has dist > 0 and O + S > 0, or when every O is 0.
 * A moment / pseudo-likelihood estimate: the reference's weights out of a gap state do not sum to 1 (gap_ext + gap_open + the
 * close's 1), so this is NOT a maximum-likelihood fit of the model as scored, and no accuracy is claimed.  A negative or
 * non-finite count or distance: PAGAN_E_ARG.                                                                                   */
int     pagan_fit_indel(int32_t n, const double *dist, const double *trans, double *indel_rate, double *gap_ext);
int  pagan_msa_n_internal(const pagan_msa *m);
int  pagan_msa_node_info(const pagan_msa *m, int32_t k, pagan_node_info *out);
/* Borrowed views (valid until pagan_msa_destroy) of what node k's alignment consumed and
 * produced: usable as a pagan_job for pagan_batch_create / the oracle.                   */
int  pagan_msa_node_job(const pagan_msa *m, int32_t k, pagan_job *out);
int  pagan_msa_node_result(const pagan_msa *m, int32_t k, pagan_result *out);
/* What the forward/backward pass left at internal node k (full_probability / sample_path).  All of these return PAGAN_E_ARG
 * for a node this process did not align (rank mode: support is not part of the exchange format) or when no pass ran.
 * node_fb: out[0] log_fwd, [1] log_bwd, [2] device ms of the two sweeps, [3] device ms of support + marginals (a batch's
 *   launches are booked at its first node, 0 at the others).
 * node_support: [n_cols] posterior of each column's own cell along the node's path, -1 at skip columns (pagan_fb_path_support).
 * node_marginals: the eight arrays of pagan_fb_site_marginals (any may be NULL); valid with full_probability == 2.
 * node_model_prob: borrowed view of the probability-space model the pass used (valid until pagan_msa_destroy).
 * support_row: node `node`'s (n_leaves .. 2 n_leaves - 2) column support laid onto the final alignment's columns, -1 where
 *   the node has no matched / xgapped / ygapped column; buf holds alignment_length floats (codons: one per column of three
 *   characters).  Leaves: PAGAN_E_ARG.                                                                                    */
int  pagan_msa_node_fb(const pagan_msa *m, int32_t k, double out[4]);
/* node_decode (pagan_msa_set_decoder): out[0] the decoded path's objective, [1] its steps, [2] device ms of the decode's fill +
 *   trace (a sub-batch's launches are booked at its first node, 0 at the others); PAGAN_E_ARG for a node this process did not align */
int  pagan_msa_node_decode(const pagan_msa *m, int32_t k, double out[3]);
int  pagan_msa_node_support(const pagan_msa *m, int32_t k, double *support);
int  pagan_msa_node_marginals(const pagan_msa *m, int32_t k, double *pX, double *pM_left, int32_t *best_j, double *best_p_left,
                              double *pY, double *pM_right, int32_t *best_i, double *best_p_right);
int  pagan_msa_node_model_prob(const pagan_msa *m, int32_t k, pagan_model_prob *out);
int  pagan_msa_support_row(const pagan_msa *m, int32_t node, float *buf);
int  pagan_msa_timing_get(const pagan_msa *m, pagan_msa_timing *out);
int  pagan_msa_alignment_length(const pagan_msa *m);
/* Row of node `node` of the final alignment, '-' for gaps; buf >= length+1.  Leaves 0..n-1 in input order;
 * internal nodes n..2n-2 (the ancestors' rows of --output-ancestors: the state's character, a gap where the
 * site is skipped or deleted; get_alignment_column_at, node.cpp:779-834).                                  */
int  pagan_msa_alignment_row(const pagan_msa *m, int32_t node, char *buf);
/* The leaf rows as FASTA, leaves in guide-tree order, `>name` + the row cut into lines of chars_by_line
 * characters (<= 0: 60): Fasta_reader::write_fasta over Node::get_alignment
 * (src/utils/fasta_reader.cpp:596-629, src/main/node.cpp:537-575).                            */
int  pagan_msa_write_fasta(const pagan_msa *m, const char *path, int32_t chars_by_line);
/* ... with include_internal != 0 every node, in Node::get_all_nodes order (left subtree, node, right subtree;
 * node.h:277-290), internal nodes named #k# (node.h:479-495): Node::get_alignment(.., true), node.cpp:537-555. */
int  pagan_msa_write_fasta_nodes(const pagan_msa *m, const char *path, int32_t chars_by_line, int32_t include_internal);
void *pagan_msa_node_graph(const pagan_msa *m, int32_t node);   /* a pagan_hgraph (borrowed)  */
void pagan_msa_destroy(pagan_msa *m);

/* ---- pileup chain (BASELINE config 1: --queryfile reads --pileup-alignment --homopolymer) -----------------
 * Reads_aligner::pileup_alignment (src/main/reads_aligner.cpp:151-264): read 0 is the reference; every further
 * read is aligned (GPU) against the current root as a temporary two-child node -- root at distance 0.001, read at
 * query_distance, reads settings (basic_alignment.h:572-586) -- and joins the alignment when
 * overlap > min_overlap and identity > min_identity (read_alignment_scores, reads_aligner.cpp:3323-3465).      */
typedef struct pagan_pileup pagan_pileup;
typedef struct pagan_pileup_opts {
    int32_t  leaf_flags;         /* 1 = --454, 2 = --homopolymer (default): leaf graphs and ins = del = 0.25 */
    uint32_t dp_flags;           /* PAGAN_OPT_*                                                           */
    float    query_distance;     /* --query-distance, default 0.1 (settings.cpp:107)                      */
    float    min_overlap;        /* --min-query-overlap, default 0.5                                      */
    float    min_identity;       /* --min-query-identity, default 0.5                                     */
    int32_t  use_anchors;        /* 0 = full matrices (default), 1 = prefix anchors                       */
    int32_t  anchors_offset, prefix_hit_length, hit_trim;
    int32_t  device;             /* HIP device, -1 = current                                              */
} pagan_pileup_opts;
typedef struct pagan_pileup_step {
    int32_t read;                /* index of the read this step tried to add                              */
    int32_t accepted;
    float   overlap, identity;   /* aligned / read_length, matched / aligned                              */
    int32_t aligned, matched, read_length;
    int32_t left_sites, right_sites, status, n_cols;
    double  score;
    int64_t cells;
} pagan_pileup_step;
void pagan_pileup_default_opts(pagan_pileup_opts *o);
int  pagan_pileup_create(int32_t n_reads, const char *const *names, const char *const *seqs,
                         const pagan_pileup_opts *opts, pagan_pileup **out);
int  pagan_pileup_align(pagan_pileup *p);
int  pagan_pileup_n_steps(const pagan_pileup *p);                              /* n_reads - 1 */
int  pagan_pileup_step_info(const pagan_pileup *p, int32_t k, pagan_pileup_step *out);
int  pagan_pileup_step_job(const pagan_pileup *p, int32_t k, pagan_job *out);  /* borrowed views */
int  pagan_pileup_step_result(const pagan_pileup *p, int32_t k, pagan_result *out);
int  pagan_pileup_alignment_length(const pagan_pileup *p);
int  pagan_pileup_alignment_row(const pagan_pileup *p, int32_t read, char *buf);   /* "" for a rejected read */
int  pagan_pileup_set_batch_backend(pagan_pileup *p, pagan_batch_fn fn, void *user);  /* TEST SEAM, as for pagan_msa */
void pagan_pileup_destroy(pagan_pileup *p);

/* ---- host graphs on their own ---------------------------------------------------------- */
typedef struct pagan_hgraph pagan_hgraph;
pagan_hgraph *pagan_hgraph_leaf(const char *residues, const char *full_alphabet, int32_t flags);
/* Sequence::create_codon_sequence (src/main/sequence.cpp:306-359): one site per triplet of the nucleotide string,
 * state 61 (NNN) for what is not a sense codon; a plain chain.  pagan_hgraph_string on such a graph (and on its
 * parents) takes the three-letter names of pagan_codon_alphabet and writes three characters per site.            */
pagan_hgraph *pagan_hgraph_leaf_codon(const char *nucleotides);
/* flags: bit0 reads/keep-all-edges settings, bit1 --no-reduced-terminal-penalties            */
pagan_hgraph *pagan_hgraph_parent(pagan_hgraph *left, pagan_hgraph *right, const pagan_result *res,
                                  float left_branch, float right_branch, const int32_t *parsimony,
                                  int32_t n_states, int32_t char_as, int32_t flags);
/* The same parent built on the current HIP device (csrc/dp_parent.hip: Basic_alignment::build_ancestral_sequence,
 * basic_alignment.cpp:36-653, as maps, scans and per-site loops).  Field for field the graph
 * pagan_hgraph_parent returns; NULL without a device or on a HIP error (never a host-built graph in its place).
 * info[5] (may be NULL): runs of skipped sites, rounds of the boundary pass's fixpoint, deleted sites, edge weights outside
 * the log-weight table, log weights the host had to correct.  The tree walk uses it for nodes of 20,000 columns and more
 * (PAGAN_PARENTS=host / device forces either); pagan_parents_device_calls counts those.                            */
pagan_hgraph *pagan_hgraph_parent_device(pagan_hgraph *left, pagan_hgraph *right, const pagan_result *res,
                                         float left_branch, float right_branch, const int32_t *parsimony,
                                         int32_t n_states, int32_t char_as, int32_t flags, int32_t *info);
long long pagan_parents_device_calls(void);
void pagan_hgraph_view(const pagan_hgraph *g, pagan_graph *out);
/* site_attr [n_sites][8] = state,type,path_state,left,right,count_since_used,ambiguous,n_fwd;
 * site_dist [n_sites]; edge_attr [n_edges][6] = start,end,used,count_since_used,
 * count_as_skipped,linked; edge_f [n_edges][3] = weight,log_weight,dist_since_used.       */
void pagan_hgraph_attrs(const pagan_hgraph *g, int32_t *site_attr, float *site_dist,
                        int32_t *edge_attr, float *edge_f);
void pagan_hgraph_fwd(const pagan_hgraph *g, int32_t *fwd_off, int32_t *fwd_eid);
int  pagan_hgraph_string(const pagan_hgraph *g, int32_t with_gaps, const char *full_alphabet, char *out);
void pagan_hgraph_free(pagan_hgraph *g);

/* Viterbi_alignment::define_tunnel for --use-prefix-anchors; upper/lower hold
 * strlen(gapped1)+1 entries.  Returns the number of anchors used.                        */
int  pagan_define_tunnel(const char *s1, const char *s2, const char *gapped1, const char *gapped2,
                         int32_t prefix_hit_length, int32_t hit_trim, int32_t offset,
                         int32_t *upper, int32_t *lower);

/* The tunnel from a list of possibly overlapping hits, the reference's BLAST branch from the hit list onwards.
 * hits: n x 4 ints (start in sequence 1, start in sequence 2, length, score), positions in the UNGAPPED strings.
 * pagan_prefix_hits: Find_anchors::find_long_substrings (find_anchors.cpp:35-127); returns the number of hits.
 * pagan_drop_bad_hits: Find_anchors::eliminate_bad_hits (find_anchors.cpp:497-545), in place, returns the count.
 * pagan_define_tunnel_overlapping: Find_anchors::define_tunnel_with_overlapping_hits (find_anchors.cpp:643-843);
 *   upper/lower hold strlen(gapped1)+1 entries; blocks (cap x 4 ints: start x, start y, end x, end y) are the empty
 *   tunnel blocks ascending by size; returns their number.
 * pagan_force_gap: Viterbi_alignment::replace_largest_tunnel_block_with_gap_tunnel (viterbi_alignment.cpp:467-553)
 *   on the last (largest) block; returns 1 if it was replaced, 0 if no block of at least `threshold` cells is left. */
int  pagan_prefix_hits(const char *s1, const char *s2, int32_t min_length, int32_t *hits, int32_t cap);
/* diagnostic: how often the prefix-anchor finder ran on the device (csrc/dp_anchors.hip: suffix array by prefix doubling on the
 * GPU; PAGAN_ANCHORS=host keeps it on the host, which is also where it runs without a device)                               */
long long pagan_anchors_device_calls(void);
/* debug seam for the tests: the list pagan_prefix_hits starts from, before its sort by length and its overlap filter -- the
 * adjacent cross-string pairs of the suffix array with a common prefix >= min_length, in suffix-array order
 * (find_anchors.cpp:66-85).  hits: cap x 3 ints (start in s1, start in s2, length); cap = strlen(s1) + strlen(s2) + 1 always
 * suffices.  Returns the number of pairs (those beyond cap are not written).  where = 0: the host's builder; where = 1: the
 * device's (csrc/dp_anchors.hip) on the calling thread's anchor device, whatever the lengths and however many finders are in
 * flight; PAGAN_E_NODEVICE where it declines (no device, a HIP error, a text of 2^20 - 1 symbols or more).  Does not count
 * as a device call in pagan_anchors_device_calls.                                                                       */
int  pagan_prefix_hits_raw(const char *s1, const char *s2, int32_t min_length, int32_t where, int32_t *hits, int32_t cap);
int  pagan_drop_bad_hits(int32_t *hits, int32_t n, int32_t thr_total, int32_t thr_partly);
int  pagan_define_tunnel_overlapping(const int32_t *hits, int32_t n, const char *gapped1, const char *gapped2, int32_t width,
                                     int32_t *upper, int32_t *lower, int32_t *blocks, int32_t cap);
int  pagan_force_gap(int32_t *upper, int32_t *lower, int32_t n, const int32_t *blocks, int32_t n_blocks, int32_t threshold,
                     int32_t width, int32_t wide);

/* DNA Evol_model for a distance: table [a + b*15] (15x15 floats), params[4] =
 * log_gap_open, log_gap_ext, log_gap_end_ext, log_non_gap; parsimony [i + j*15].          */
int  pagan_dna_model(const float base_freq[4], double distance, float *table, float *params,
                     int32_t *parsimony);
/* Protein (WAG) Evol_model for a distance: table [a + b*211] (211x211 floats), params as above,
 * parsimony [i + j*211] (model_factory.cpp:304-541, 1478-1595, 1871-1960, 2155-2219).              */
int  pagan_protein_model(double distance, float *table, float *params, int32_t *parsimony);
/* Codon (Kosiol & Goldman's empirical model) Evol_model for a distance: 1892 states = 61 sense codons, NNN,
 * 1830 codon pairs; table [a + b*1892], params as above, parsimony [i + j*1892]
 * (Model_factory::define_codon_alphabet / codon_model / alignment_model, model_factory.cpp:839-1217, 1599-1805,
 * 1871-1960, 2022-2092).                                                                                       */
int  pagan_codon_model(double distance, float *table, float *params, int32_t *parsimony);
/* names: 3 characters per state (>= 3*1892 + 1 bytes) -- what a state prints as (the ancestral character
 * alphabet, model_factory.cpp:1739-1803; its first 62 entries are the leaf alphabet, model_factory.h:209-221);
 * mostcommon [i + j*61] (model_factory.cpp:1208-1217).  Either may be NULL.  Returns the number of states.      */
int  pagan_codon_alphabet(char *names, int32_t *mostcommon);
/* Codon_translation::gapped_DNA_to_protein (src/utils/codon_translation.cpp:32-107): one amino-acid letter per triplet of
 * a codon string ("---" -> '-', X for what the table does not hold) -- the strings the anchors of a codon walk are found in
 * (viterbi_alignment.cpp:54-60, 141-145).  out holds strlen/3 + 2 bytes.  Returns the number of letters.               */
int  pagan_codon_translate(const char *codons, char *out);
/* Leaf states of a nucleotide string read as codons (sequence.cpp:318-336); states holds (strlen+2)/3 entries.
 * Returns the number of states.                                                                                */
int  pagan_codon_states(const char *nucleotides, int32_t *states);
/* The same model in probability space, what the forward/backward pass takes (pagan_model_prob):
 * score [a + b*S] = Evol_model::score, params[3] = gap_open, gap_ext, non_gap.  data_type 1 DNA, 2 protein,
 * 3 codon.                                                                                                    */
int  pagan_model_prob_table(int32_t data_type, const float *base_freq, double distance, float *score, float *params);
/* Alphabets of a data type (1 DNA, 2 protein): leaf_alphabet (state = position of the residue,
 * Sequence::full_char_alphabet) and ancestral_alphabet (the character an internal state prints as,
 * Model_factory::ancestral_character_alphabet); both >= 212 bytes.  Returns the number of states.  */
int  pagan_model_alphabets(int32_t data_type, char *leaf_alphabet, char *ancestral_alphabet);
/* Eigen::eigenQREV (src/utils/eigen.cpp:48-128) for a row-major n x n reversible rate matrix:
 * Q = U diag(root) V.  Exposed for the tests.                                                     */
int  pagan_eigen_qrev(const double *Q, const double *pi, int32_t n, double *root, double *U, double *V);

/* ---- guide tree from the sequences alone: k-mer distances on the device, UPGMA on the host --------------------
 * (csrc/dp_guide.hip, csrc/host_guide.cpp; DESIGN.md "Guide tree").  The reference leaves this to external programs.
 *
 * Cleaning: exactly pagan_msa_create's -- upper case; '-', CR, LF dropped; data_type 0 guesses as the walk does, 1 DNA,
 * 2 protein, 3 codon (read as DNA over its nucleotides); DNA U -> T, protein U -> X; letters outside the full alphabet dropped.
 * k-mer: a window of k consecutive cleaned letters, all of them core letters (ACGT / the 20 amino acids); any other window
 * contributes nothing.  2 bits a letter for DNA (k <= 31), 5 bits for protein (k <= 12), packed in a u64; "no k-mer here" is
 * all ones, which no code takes.  k = 0: pagan_guide_kmer_length of the longest cleaned sequence.
 * Distance of x, y with k-mer multisets n_x, n_y: S = sum_t min(n_x(t), n_y(t)) (an integer), m = min(|n_x|, |n_y|),
 * F = S / m (0 when m = 0), p = 1 - F^(1/k) (1 when F = 0; d = 0 when p = 0); DNA / codon: p <= 0.7, d = -0.75 ln(1 - p / 0.75);
 * protein: p <= 0.85, d = -ln(1 - p - 0.2 p^2).  fp64 on the host from the integers the device counted.
 *
 * Limits (refused with PAGAN_E_ARG before anything is allocated): n <= PAGAN_GUIDE_MAX_SEQS (the number of pairs
 * n (n - 1) / 2 stays below 2^31: a pair's sum is addressed with its index, and the pair kernel's launch is at most 2^20
 * workgroups that stride over the pairs, so no launch dimension depends on n), cleaned letters in total <=
 * PAGAN_GUIDE_MAX_POSITIONS (32-bit positions, a thread a position).  The device entries run on the caller's current device and
 * leave it current; without a device they return PAGAN_E_NODEVICE (there is no host path); a HIP error on a device that is
 * there is PAGAN_E_NOMEM (out of memory) or PAGAN_E_INTERNAL.                                                         */
#define PAGAN_GUIDE_MAX_SEQS       65536
#define PAGAN_GUIDE_MAX_POSITIONS  2147483000LL
#define PAGAN_GUIDE_PAIR_CHUNK     64      /* list entries a wave of the pair kernel takes at a time */
typedef struct pagan_guide_info {
    int32_t k;                   /* the k used                                                                   */
    int32_t data_type;           /* 1 DNA, 2 protein, 3 codon: what 0 was resolved to                            */
    int32_t pair_chunk;          /* PAGAN_GUIDE_PAIR_CHUNK                                                       */
    int32_t waves_per_pair;      /* waves of the workgroup that owns a pair's sum                                */
    int64_t positions;           /* cleaned letters in total = keys packed and sorted                            */
    int64_t entries;             /* (code, count) entries of all lists                                           */
    int64_t pairs;               /* n (n - 1) / 2                                                                */
    int64_t device_bytes;        /* what the call allocated on the device                                        */
    double  pack_ms, sort_ms, compress_ms, pairs_ms;   /* device time of the stages (events around their launches; no stage
                                                          waits for the host)                                      */
    double  upgma_ms;            /* host time of the tree builder (pagan_guide_tree), 0 otherwise                */
} pagan_guide_info;
/* shared [n * n]: S(x, y), the diagonal |n_x|; kmers [n]: |n_x|; dist [n * n]: d, the diagonal 0.  Any of the three may be NULL. */
int     pagan_guide_distances(int32_t n, const char *const *seqs, int32_t data_type, int32_t k, int64_t *shared, int64_t *kmers,
                              double *dist, pagan_guide_info *info);
/* The distances, then pagan_guide_upgma.  Returns the bytes the string needs with its NUL (> cap: nothing was written, call
 * again with that much) or a negative code.                                                                             */
int64_t pagan_guide_tree(int32_t n, const char *const *names, const char *const *seqs, int32_t data_type, int32_t k,
                         char *newick_out, int64_t cap, pagan_guide_info *info);
/* Host only.  kmer_length: the smallest k with A^k >= 16 max_len (A = 4 for data_type 1 and 3, 20 for 2), clamped to 8..31
 * resp. 3..12; PAGAN_E_ARG for another data_type or max_len < 0.  distance_of: d from S, m, k as above, NaN for arguments
 * outside 0 <= S <= m, 1 <= k <= 31 resp. 12, data_type 1..3.                                                          */
int     pagan_guide_kmer_length(int32_t data_type, int64_t max_len);
double  pagan_guide_distance_of(int64_t shared, int64_t m, int32_t k, int32_t data_type);
/* UPGMA over dist [n * n] (read at [i * n + j], i < j; finite, >= 0).  Leaves are clusters 0..n-1, the cluster of step t is
 * n + t; a step merges the active pair of smallest distance (ties: lowest first id, then lowest second id), height d / 2, the
 * distance to every other active c is (n_a d(a,c) + n_b d(b,c)) / (n_a + n_b) in exactly that form, the left child is the
 * lower id, a branch is max(0, h(parent) - h(child)) printed %.17g.  Names that are empty or hold any of "(),:;" or white
 * space: PAGAN_E_ARG (pagan_msa_create's reader could not read them back).  Returns as pagan_guide_tree.                 */
int64_t pagan_guide_upgma(int32_t n, const char *const *names, const double *dist, char *newick_out, int64_t cap);
/* Device bytes pagan_guide_distances allocates for n sequences of total_len cleaned letters in total: exact for the call's own
 * buffers (the lists are sized for one entry per position), an ESTIMATE for the sort's and the scan's temporary storage (a
 * second key buffer, index arrays over the sequences, 1 MiB: what rocPRIM asks for is known only with a device, and a call takes
 * that if it is more; pagan_guide_info.device_bytes is what a call did allocate).  PAGAN_E_ARG beyond the limits above.    */
int64_t pagan_guide_predict_bytes(int32_t n, int64_t total_len);

/* ---- guide tree from an alignment: row pair counts on the device, the same distance, the same UPGMA -----------------
 * (csrc/dp_alndist.hip, csrc/host_guide.cpp; DESIGN.md "Guide tree from the alignment").  The step back from a first
 * alignment to a tree: the reference takes it with external programs (--bppdist-tree, --raxml-tree).
 *
 * Input: n rows of the same length L (a ragged set: PAGAN_E_ARG; L = 0 is allowed).  data_type 0, 1, 2, 3 is resolved as the
 * guide's cleaning resolves it, over the rows with their gap characters dropped; a codon alignment (3) is read as DNA over its
 * nucleotide characters (the walk's codon rows hold three characters a column).
 * Letters: a character is upper-cased and a DNA U counts as T.  It is a letter if it is a core letter -- ACGT, or the 20 amino
 * acids in the order ARNDCQEGHILKMFPSTWYV -- and its code is its position in that list.  Everything else is no letter: '-',
 * '.', N, X, ambiguity codes, anything.  Unlike the sequence cleaner nothing is dropped: a column keeps its place.
 * Counts: both(x, y) = the columns where row x and row y each hold a letter; match(x, y) = those of them where the two codes are
 * equal; both(x, x) = match(x, x) = the letters of row x.  Integers, exact whatever the order of summation.
 * Distance: d(x, y) = pagan_guide_distance_of(match, both, 1, data_type) for x != y (p = 1 - match / both with that function's
 * clamps and formulas; both = 0 gives the clamp's distance, as "nothing shared" does for k-mers), 0 on the diagonal.
 * Tree: pagan_guide_upgma over that matrix.
 *
 * Limits (PAGAN_E_ARG before anything is allocated): 2 <= n <= PAGAN_GUIDE_MAX_SEQS, L < 2^31 (a count is a uint32 on the
 * device).  Device, errors: as for the guide tree above -- the caller's current device, left current; PAGAN_E_NODEVICE without
 * one (there is no host path); PAGAN_E_NOMEM / PAGAN_E_INTERNAL for a HIP error.                                              */
#define PAGAN_ALN_TILE         64      /* rows a side of the tile of pairs a workgroup owns                               */
#define PAGAN_ALN_SPLIT_WORDS  8       /* words (of 64 columns) of the granule a tile's columns are split in              */
typedef struct pagan_aln_info {
    int32_t data_type;           /* 1 DNA, 2 protein, 3 codon: what 0 was resolved to                            */
    int32_t planes;              /* bit planes a row is packed in: valid + 2 (DNA, codon) or + 5 (protein) code bits */
    int32_t tile;                /* PAGAN_ALN_TILE                                                               */
    int32_t col_splits;          /* workgroups that share the words of one tile (1: no partial sums, no fold)    */
    int64_t columns;             /* L                                                                            */
    int64_t words;               /* ceil(L / 64)                                                                 */
    int64_t pairs;               /* n (n - 1) / 2                                                                */
    int64_t device_bytes;        /* what the call allocated on the device                                        */
    double  pack_ms, pairs_ms;   /* device time of the stages (events around their launches; pairs_ms includes the fold; no
                                    stage waits for the host)                                                    */
    double  upgma_ms;            /* host time of the tree builder (pagan_aln_tree, pagan_msa_alignment_tree), 0 otherwise */
} pagan_aln_info;
/* both, match, dist: [n * n], both triangles and the diagonal filled.  Any of the three may be NULL. */
int     pagan_aln_distances(int32_t n, const char *const *rows, int32_t data_type, int64_t *both, int64_t *match, double *dist,
                            pagan_aln_info *info);
/* The distances, then pagan_guide_upgma.  Returns what pagan_guide_tree returns, under the same contract. */
int64_t pagan_aln_tree(int32_t n, const char *const *names, const char *const *rows, int32_t data_type, char *newick_out,
                       int64_t cap, pagan_aln_info *info);
/* Host only.  Device bytes pagan_aln_distances allocates for n rows of `columns` columns: exact for the call's own buffers of a
 * protein alignment (6 planes); a DNA or codon call packs 3 planes and takes less (pagan_aln_info.device_bytes is what a call
 * did allocate, never more than this).  PAGAN_E_ARG beyond the limits above.                                              */
int64_t pagan_aln_predict_bytes(int32_t n, int64_t columns);
/* pagan_aln_tree over the leaf rows of a finished walk, under the walk's names and data type.  PAGAN_E_ARG before the rows
 * exist (a walk not yet aligned / finished).                                                                              */
int64_t pagan_msa_alignment_tree(const pagan_msa *m, char *newick_out, int64_t cap, pagan_aln_info *info);

/* ---- ancestral states by marginal likelihood: pruning up the tree, the outside pass down, on the device --------------
 * (csrc/dp_anc.hip, csrc/host_anc.cpp; DESIGN.md "Ancestral states").  The reference leaves this to the external program
 * bppancestor (src/utils/bppancestors.cpp:98-317) and overlays its states on the ancestors' rows.
 *
 * Model: the walk's substitution model over its core states -- data_type 1 DNA (S = 4, ACGT), 2 protein (S = 20, WAG,
 * ARNDCQEGHILKMFPSTWYV), 3 codon (S = 61, the empirical codon model, the sense codons in pagan_codon_alphabet's order).
 * P(t)[i][j] = max(0, sum_k U[i,k] exp(t root[k]) V[k,j]) with k outermost in fp64, the sum the alignment model takes; it is not
 * renormalised; t = 0 gives the exact identity.  U, V, root are the eigen solution of the model's rate matrix made a proper one:
 * the reference's matrices (float products for DNA, a table of decimal literals for codons) are reversible under pi and have zero
 * row sums only to the digits they carry, which a log-odds table does not mind and a likelihood does (rows of P off 1 by up to
 * 6.6e-5); so the exchange flows pi_i q_ij are averaged with their mirror images and the diagonal is set to minus the row's sum
 * before pagan_eigen_qrev's solver runs (pagan_anc_rate_matrix returns that matrix).  Rows of P then sum to 1, and pi_i P_ij = pi_j P_ji, to a few 1e-15.  The alignment
 * model itself (pagan_dna_model and the others) is unchanged.
 * Tree: n leaves 0 .. n-1, internal node n + k (k = 0 .. n-2) with children left[k], right[k], both ids < n + k (the walk's ids:
 * children before parents, the root is 2n - 2); every node but the root is a child exactly once; branch[2n-1] is the length
 * above each node, finite and >= 0, the root's entry ignored.  Anything else: PAGAN_E_TREE.
 * Leaf encoding: n rows of equal length (pagan_aln_distances' checks and its resolution of data_type 0).  A character is
 * upper-cased and a DNA U counts as T.  DNA: the 15 IUPAC letters ACGTRYMKWSBDHVN are state sets (R = AG, Y = CT, M = AC, K = GT,
 * W = AT, S = CG, B = CGT, D = AGT, H = ACT, V = ACG, N = ACGT); anything else ('-', '.', '?', other letters) is missing data, the
 * all-ones vector.  Protein: the 20 letters are states; everything else is missing, X, B, Z and U included.  Codon: a column is
 * three characters (a row length that is no multiple of 3: PAGAN_E_ARG); a triplet pagan_codon_states reads as one of the 61
 * sense codons is that state; anything else is missing -- NNN, "---", stop codons, partial gaps.
 * Computation: up, L_v[s] = a[s] b[s], a[s] = sum_t P_left[s][t] L_left[t] with t ascending (b likewise); a leaf's L is the
 * indicator of its state set; a child none of whose leaves holds data in the column contributes the exact factor 1.  After every
 * node with data below it the vector is multiplied by 2^-e, e the binary exponent of its largest entry (ldexp: exact), and e is added to the column's
 * int32.  Root: col_lik = sum_s pi[s] L_root[s], s ascending (the exact 1 for a column without any data).  Down, O_root = pi; for child c of v with sibling b,
 * W[s] = O_v[s] m_b[s] (m_b the sibling's message a or b above), O_c[t] = sum_s W[s] P_c[s][t] with s ascending, rescaled the
 * same way.  Posterior of v: q[s] = L_v[s] O_v[s] divided by sum_s q[s] (s ascending; all zero where that sum is zero).  Tie rule
 * of `best`: the first maximum in state order (a later state replaces it only when strictly larger); in a column that cannot
 * happen (likelihood 0, every q[s] zero) that is state 0, with best_p 0.  Every sum has a fixed
 * order and no contraction: the outputs are bit-identical from run to run and for every chunk size.
 * The device works on chunks of columns (pagan_anc_info.chunk_cols, a multiple of 64), so its footprint is bounded by the chunk,
 * not by the alignment; PAGAN_ANC_CHUNK_COLS in the environment forces the chunk size.  Device, errors: as for the guide trees
 * above -- the caller's current device, left current; PAGAN_E_NODEVICE without one (there is no host path).                    */
#define PAGAN_ANC_MAX_STATES 61
typedef struct pagan_anc_info {
    int32_t data_type;           /* 1 DNA, 2 protein, 3 codon: what 0 was resolved to                            */
    int32_t states;              /* S                                                                            */
    int32_t chunks;              /* column chunks the call ran                                                   */
    int32_t matrices;            /* distinct branch lengths = transition matrices uploaded                       */
    int64_t columns;             /* L (codons: row length / 3)                                                   */
    int64_t chunk_cols;          /* columns of a chunk                                                           */
    int64_t device_bytes;        /* what the call allocated on the device                                        */
    double  encode_ms, up_ms, down_ms;   /* device time of the stages, summed over the chunks (events around the launches) */
} pagan_anc_info;
/* Host only.  P [S * S] row-major and pi [S] (either may be NULL) of data_type 1 / 2 / 3 for branch length t; base_freq (DNA
 * only, NULL: 0.25 each) as pagan_dna_model takes it, kappa and rho at the walk's defaults.  Returns S, or PAGAN_E_ARG (another
 * data_type, t negative or not finite), PAGAN_E_INTERNAL where the eigen solver fails.                                       */
int     pagan_anc_pmatrix(int32_t data_type, const float *base_freq, double t, double *P, double *pi);
/* Host only.  The rate matrix pagan_anc_pmatrix exponentiates, Q [S * S] row-major, and pi [S] (either may be NULL): from the
 * model's rates q (pagan_dna_model's HKY matrix as the reference builds it, in float arithmetic; the WAG table; the empirical
 * codon table) r_ij = (pi_i q_ij + pi_j q_ji) / 2 / pi_i for i != j and r_ii = -(sum of the row's other entries, in column
 * order).  Returns S, or PAGAN_E_ARG.                                                                                      */
int     pagan_anc_rate_matrix(int32_t data_type, const float *base_freq, double *Q, double *pi);
/* Host only.  The leaf codes of one row by the tables the device encodes with: codes [strlen(row)] (codons: / 3; a length that
 * is no multiple of 3: PAGAN_E_ARG).  DNA: the state set as bits (1 A, 2 C, 4 G, 8 T), 0 for missing data; protein, codon: the
 * state, 255 for missing data.  codes may be NULL.  Returns the number of columns.                                            */
int64_t pagan_anc_encode_row(int32_t data_type, const char *row, uint8_t *codes);
/* Host only.  PAGAN_OK or PAGAN_E_TREE (PAGAN_E_ARG: n < 2 or a null array) by the tree rules above. */
int     pagan_anc_check_tree(int32_t n_leaves, const int32_t *left, const int32_t *right, const double *branch);
/* Host only.  Device bytes of a pagan_anc_reconstruct call over n_leaves rows of `columns` columns in chunks of chunk_cols
 * (<= 0: what the call itself would take, PAGAN_ANC_CHUNK_COLS included): exact for the call's own buffers when every branch
 * length is distinct and every internal node's posterior is asked for; a call with fewer of either takes less
 * (pagan_anc_info.device_bytes is what a call did allocate, never more than this).  PAGAN_E_ARG beyond the limits.        */
int64_t pagan_anc_predict_bytes(int32_t n_leaves, int64_t columns, int32_t data_type, int64_t chunk_cols);
/* rows: n_leaves rows of L characters (codons: 3 L).  flags: 0 (reserved).  post_nodes [n_post]: ids n .. 2n-2 of the internal
 * nodes whose full posterior vectors are wanted.  Outputs, any may be NULL:
 *   col_lik [L], col_exp [L]   the column's likelihood as the device left it: col_lik * 2^col_exp
 *   col_loglik [L]             log(col_lik) + col_exp * ln 2, taken on the host
 *   loglik                     col_loglik[0] + col_loglik[1] + ..., left to right in fp64: exactly that sum
 *   best, best_p [(n-1) * L]   row k: internal node n + k's state of largest posterior in each column, and that posterior
 *   has_data [(2n-1) * L]      bytes: 1 where any leaf below the node holds a non-missing character in the column
 *   post [n_post * L * S]      the posterior vectors of the listed nodes                                                      */
int     pagan_anc_reconstruct(int32_t n_leaves, const int32_t *left, const int32_t *right, const double *branch,
                              const char *const *rows, int32_t data_type, const float *base_freq, uint32_t flags,
                              int32_t n_post, const int32_t *post_nodes, double *col_lik, int32_t *col_exp, double *col_loglik,
                              double *loglik, uint8_t *best, float *best_p, uint8_t *has_data, double *post, pagan_anc_info *info);
/* The reconstruction over a finished walk: its leaf rows, its tree and the branch lengths it ALIGNED under -- the corrected,
 * truncated lengths (Node::set_distance_to_parent: <= 0 becomes 0.001, anything above truncate_branches is cut to it), not the
 * input tree's -- and for DNA its empirical base frequencies.  The result is kept in the handle for the three readers below.
 * col_loglik (alignment_length, codons / 3, doubles) and info may be NULL.  PAGAN_E_ARG before the rows exist.
 * ancestral_row: pagan_msa_alignment_row's row with every non-gap character of an internal node replaced by the letter of `best`
 *   (codons: the three characters of the codon) -- the reference's overlay, bppancestors.cpp:242-254: gaps stay gaps, PAGAN's indel
 *   pattern is kept; leaves come back unchanged.  The reference's copy of the root's characters from its nearer child
 *   (:273-314, bppancestor works on an unrooted tree) is NOT restated: this pass is rooted and the root has its own posterior.
 * ancestral_support: the posterior of the shown state per column (codons: per triplet), -1 at gaps; leaves: PAGAN_E_ARG.
 * write_fasta_ancestral: pagan_msa_write_fasta_nodes(.., 1)'s file with the overlaid rows.
 * All three return PAGAN_E_ARG before pagan_msa_ancestral has run.                                                          */
int     pagan_msa_ancestral(pagan_msa *m, uint32_t flags, double *loglik, double *col_loglik, pagan_anc_info *info);
int     pagan_msa_ancestral_row(const pagan_msa *m, int32_t node, char *buf);
int     pagan_msa_ancestral_support(const pagan_msa *m, int32_t node, float *buf);
int     pagan_msa_write_fasta_ancestral(const pagan_msa *m, const char *path, int32_t chars_by_line);
/* Borrowed views (valid until the next pagan_msa_ancestral or pagan_msa_destroy) of the kept best [(n-1) * L] and best_p. */
int     pagan_msa_ancestral_best(const pagan_msa *m, const uint8_t **best, const float **best_p);

/* ---- branch lengths by maximum likelihood: the derivatives of the log likelihood on the device, the fit on the host ---
 * (csrc/dp_anc_brlen.inc, csrc/host_anc.cpp; DESIGN.md "Branch lengths by maximum likelihood").  The reference takes its branch
 * lengths from external programs (bppdist, raxml, fasttree: src/utils/bppdist_tree.*, raxml_tree.*, fasttree_tree.*); none of
 * that is restated.
 *
 * The model, the tree rules, the leaf encoding, P(t), L, O, m_b, W and the rescaling are exactly those of "ancestral states by
 * marginal likelihood" above; the two passes are that section's, unchanged.
 * Derivative matrices: D_r(t)[i][j] = sum_k U[i,k] root[k]^r exp(t root[k]) V[k,j], k outermost, in fp64, for r = 1, 2, NOT clamped
 * (root[k]^2 is root[k] * root[k]; the factor root[k]^r exp(t root[k]) is formed first, then times U[i,k], then times V[k,j]).  D_0 is
 * pagan_anc_pmatrix's P(t) itself, clamp included, so f_0 below is the likelihood the up pass computes.
 * Per branch and column: c any node but the root, v its parent, b its sibling.  y_r[s] = sum_t D_r(t_c)[s][t] L_c[t], t ascending
 * (a leaf's L_c: the indicator of its state set); f_r = sum_s W[s] y_r[s], s ascending, W[s] = O_v[s] m_b[s], O_root = pi.  The
 * column is informative for c when has_data[c] is set, some leaf outside c's subtree holds data -- a flag carried down the tree:
 * out_has[root] = false, out_has[c] = out_has[v] || has_data[b] -- and f_0 > 0.  An informative column contributes f_1 / f_0 to
 * g1[c] and f_2 / f_0 - (f_1 / f_0)^2 to g2[c]; every other column contributes the exact 0.  informative[c] counts them.  L and O
 * enter as the passes left them: the powers of two of the rescaling cancel in the quotients and are never applied.
 * Order of the column sum: columns 64 q .. 64 q + 63 of the alignment are block q (columns past the end contribute 0).  Within a
 * block x[i] is column 64 q + i's contribution, and for d = 32, 16, 8, 4, 2, 1 in turn x[i] = x[i] + x[i + d] for all i < d; the
 * block's sum is x[0].  The blocks are then added left to right, sum = sum + block q for q = 0, 1, ..., from 0.  Chunks are
 * multiples of 64 columns, so g1 and g2 are the same bytes from run to run and for every chunk size.
 * The root: its two branches are one parameter tau = t_l + t_r (the pulley principle: the model is reversible).  The device
 * reports the sums of both children; the fit uses the left child's for tau, keeps tau within [t_min, t_max] like any branch and
 * splits it as t_l = tau p, t_r = tau - t_l with p = t_l / (t_l + t_r) of branch_in (1/2 where both are 0).
 * Step rule (pagan_anc_branch_step): non-finite t, g1 or g2, or g1 == 0 && g2 == 0 (no information): t.  Otherwise s = t - g1 / g2
 * where g2 < 0 (Newton), else 2 t where g1 > 0, else t / 2; s is kept within [t / 4, 4 t], then within [t_min, t_max].
 * Fit: the lengths start from branch_in, every parameter kept within [t_min, t_max].  One up pass gives their loglik.  A round:
 * the down pass, g1 / g2 of all branches at once, the step of all parameters at once.  Where max |t' - t| / max(t, t_min) over
 * the parameters is <= tol the fit stops CONVERGED at t.  Otherwise the candidate t + alpha (t' - t) (alpha = 1: t' itself) gets
 * an up pass of its own, alpha = 1, 1/2, ..., 1/32; the first whose loglik is not lower than the accepted one is accepted and
 * the next round starts from it; none: STALLED at t.  After max_rounds rounds: MAX_ROUNDS.  The accepted logliks never decrease,
 * and each is bit for bit pagan_anc_reconstruct's loglik at those lengths.
 * The rows are uploaded and encoded once a call and their codes stay on the device; the partials and outside vectors are kept
 * for one chunk (PAGAN_ANC_CHUNK_COLS as above).  Device, errors: as for pagan_anc_reconstruct -- no host path.               */
#define PAGAN_ANC_FIT_CONVERGED  0
#define PAGAN_ANC_FIT_MAX_ROUNDS 1
#define PAGAN_ANC_FIT_STALLED    2
typedef struct pagan_anc_fit_opts {
    double  t_min, t_max;        /* bounds of every parameter: 1e-6, 10; 0 < t_min <= t_max                      */
    double  tol;                 /* the relative change that counts as none: 1e-6; >= 0                          */
    int32_t max_rounds;          /* 32; >= 0                                                                     */
    int32_t reserved;            /* 0                                                                            */
} pagan_anc_fit_opts;
typedef struct pagan_anc_fit_info {
    int32_t status;              /* PAGAN_ANC_FIT_*                                                              */
    int32_t rounds;              /* derivative evaluations made                                                  */
    int32_t up_passes;           /* up passes over the whole alignment, retries included                         */
    int32_t chunks;              /* column chunks of one pass                                                    */
    int32_t data_type, states;   /* as pagan_anc_info                                                            */
    int64_t columns, chunk_cols;
    int64_t device_bytes;        /* what the call allocated on the device                                        */
    double  loglik_start, loglik_end;    /* of the lengths the fit started from and of those it returns          */
    double  encode_ms, up_ms, down_ms, branch_ms, fold_ms;   /* device time of the stages, summed over the call  */
    double  total_ms;            /* host wall time of the call: what exceeds the stages is the host's share      */
} pagan_anc_fit_info;
/* Host only.  D_order(t) [S * S] row-major, order 1 or 2, as defined above.  Returns S, or PAGAN_E_ARG as pagan_anc_pmatrix
 * does and for another order.                                                                                              */
int     pagan_anc_pmatrix_deriv(int32_t data_type, const float *base_freq, double t, int32_t order, double *D);
/* Host only, plain arithmetic: the step rule above. */
double  pagan_anc_branch_step(double t, double g1, double g2, double t_min, double t_max);
/* One evaluation on the device: g1, g2 [2n-1] and informative [2n-1] by node id, the root's entries 0; loglik as
 * pagan_anc_reconstruct's.  Any output may be NULL.  info: rounds 1, up_passes 1, status 0.                               */
int     pagan_anc_branch_derivs(int32_t n_leaves, const int32_t *left, const int32_t *right, const double *branch,
                                const char *const *rows, int32_t data_type, const float *base_freq, double *g1, double *g2,
                                int64_t *informative, double *loglik, pagan_anc_fit_info *info);
/* The fit.  opts NULL: the defaults; PAGAN_E_ARG for bounds, a tolerance or a round count outside the ranges above.
 * branch_out [2n-1] (the root's entry 0).  loglik_hist [hist_cap] (may be NULL): the accepted logliks, the start first; the
 * call returns how many there are (rounds accepted + 1; only the first hist_cap are written), or a negative code.             */
int     pagan_anc_fit_branches(int32_t n_leaves, const int32_t *left, const int32_t *right, const double *branch_in,
                               const char *const *rows, int32_t data_type, const float *base_freq, const pagan_anc_fit_opts *opts,
                               double *branch_out, double *loglik_hist, int32_t hist_cap, pagan_anc_fit_info *info);
/* Host only.  Device bytes of a pagan_anc_fit_branches or pagan_anc_branch_derivs call, under pagan_anc_predict_bytes' contract:
 * exact when every branch length is distinct, never less than what a call allocates.                                          */
int64_t pagan_anc_fit_predict_bytes(int32_t n_leaves, int64_t columns, int32_t data_type, int64_t chunk_cols);
/* The fit over a finished walk: its leaf rows, its tree, for DNA its base frequencies as pagan_msa_ancestral takes them, starting
 * from the lengths the walk aligned under.  branch_out [2n-1] by node id (may be NULL).  newick_out: the walk's topology and
 * names with the fitted lengths printed %.17g; returns the bytes the string needs with its NUL (> cap: the string was not
 * written, the rest was), or a negative code.  The walk itself is not changed.  PAGAN_E_ARG before the rows exist.            */
int64_t pagan_msa_fit_branches(const pagan_msa *m, const pagan_anc_fit_opts *opts, double *branch_out, char *newick_out,
                               int64_t cap, pagan_anc_fit_info *info);

/* ---- tree search by nearest-neighbour interchange: the gains of every edge at once on the device, the search on the host --
 * (csrc/dp_anc_nni.inc, csrc/host_anc.cpp; DESIGN.md "Tree search by nearest-neighbour interchange").  The reference gets its
 * likelihood trees from external programs (raxml, fasttree: src/utils/raxml_tree.*, fasttree_tree.*); none of that is restated.
 *
 * The model, the tree rules, the leaf encoding, P(t), L, O, the message and the rescaling are exactly those of "ancestral states by
 * marginal likelihood" above: m_x[s] = sum_t P(t_x)[s][t] L_x[t], t ascending, the exact 1 for a child without data.  The two passes
 * are that section's, unchanged.
 * Candidates, by internal node c = n + k.  Ordinary: c is internal and its parent v is not the root; a = left[c], d = right[c], b
 * is c's sibling; T[s] = O_v[s], P_mid = P(t_c).  Root edge: both children rl = left[root], rr = right[root] of the root are
 * internal; one candidate, at c = rl; a = left[rl], d = right[rl], e = left[rr], b = right[rr]; T[s] = pi[s] * m_e[s],
 * P_mid = pagan_anc_pmatrix(t_rl + t_rr), one matrix made on the host like any other (with the model's reversibility this is full
 * pruning of the rearranged tree; the three arrangements share P_mid and are consistent with one another).  Every other internal
 * node has no candidate: a swap around a child of the root whose sibling is a leaf, or around the root, only re-roots the tree.
 * Per column, for the arrangement k = 0 (as is), k = 1 (a and b exchanged), k = 2 (d and b exchanged):
 *   u_0[t] = m_a[t] * m_d[t], u_1[t] = m_b[t] * m_d[t], u_2[t] = m_a[t] * m_b[t];  X_0 = m_b, X_1 = m_a, X_2 = m_d;
 *   y_k[s] = sum_t P_mid[s][t] u_k[t], t ascending from 0 -- and the exact 1 for every s where neither of the two nodes u_k is
 *   made of holds data in the column: they are the children of a node without data, which contributes the exact factor 1 as it
 *   does in the up pass (rows of P sum to 1 only to a few 1e-15);  f_k = sum_s (T[s] * X_k[s]) * y_k[s], s ascending from 0.
 * L and O enter as the passes left them: every f_k holds each vector once, so the powers of two cancel in the quotient and are
 * never applied.  Ratio, k = 1, 2: where f_0 > 0 and f_k > 0, r_k = f_k / f_0; otherwise r_k is the exact 1 and the column counts
 * in degenerate[c][k].  Columns past the end of the alignment give the exact 1 and count nowhere.
 * Column product, without a logarithm on the device: (m, e) = frexp(r).  Columns 64 q .. 64 q + 63 are block q; for d = 32, 16, 8,
 * 4, 2, 1 in turn and every i < d: m[i] = m[i] * m[i + d], (m[i], de) = frexp(m[i]), e[i] = e[i] + e[i + d] + de; the block's pair
 * is (m[0], e[0]).  The blocks are multiplied left to right in the same way onto a running pair (M, E) that starts at (0.5, 1):
 * M = M * m_q, (M, de) = frexp(M), E = E + e_q + de.  The running pair survives from chunk to chunk, so (M, E) is the same bytes
 * for every chunk size.  On the host gain[c][k] = log(M) + E * log(2): the log likelihood of arrangement k minus that of the tree
 * as it is, at the branch lengths as they are.
 * Applying a swap (host only): branch[] is indexed by node id and does not change -- lengths travel with their subtrees.  k = 1
 * puts b into c's left slot and a into the slot b had; k = 2 does the same with c's right slot and d.  The internal nodes are then
 * renumbered in post-order (left subtree, right subtree, the node; leaves keep their ids), so that children come before parents
 * again and the root is 2n - 2; perm[old id] = new id.
 * Selecting swaps (host only, arithmetic on the gains): a candidate's better k is 1 unless gain[c][2] > gain[c][1]; it qualifies
 * when degenerate is 0 for that k and that gain exceeds min_gain.  The qualifying candidates are taken in order of descending gain
 * (ties: the lower c first); one is skipped when an endpoint of its edge -- {c, v}, for the root edge {rl, rr, root} -- belongs to
 * an edge already taken.
 * Search: the up pass gives ll of the start tree.  A round: the down pass, the gains, the selection.  Nothing selected: CONVERGED.
 * Otherwise all selected swaps are applied (their edges share no node, so they are applied on the round's ids in the order
 * selected and renumbered once) and an up pass gives the new tree's loglik; where that is lower than ll, the first selected swap
 * is applied alone (its gain is the exact difference up to rounding), and where that is lower too the search ends STALLED at the
 * round's start tree.  With fit_rounds > 0 the accepted tree's lengths then get pagan_anc_fit_branches' own loop, capped at
 * fit_rounds rounds, and ll becomes its loglik_end -- unless that is lower than ll, which only the fit's start can cause (it
 * first brings every length within [t_min, t_max]): then the tree keeps the lengths it has.  After max_rounds rounds: MAX_ROUNDS.  The accepted logliks never decrease,
 * and with fit_rounds = 0 each is bit for bit pagan_anc_reconstruct's loglik of that tree.
 * The rows are uploaded and encoded once a call; when the tree changes, the node table, the candidate table and the matrices are
 * uploaded again.  Device, errors: as for pagan_anc_fit_branches -- no host path.                                              */
#define PAGAN_ANC_NNI_CONVERGED  0
#define PAGAN_ANC_NNI_MAX_ROUNDS 1
#define PAGAN_ANC_NNI_STALLED    2
typedef struct pagan_anc_nni_opts {
    double  min_gain;            /* a swap must gain more than this: 1e-3; >= 0                                  */
    double  t_min, t_max, tol;   /* of the fit (pagan_anc_fit_opts): 1e-6, 10, 1e-6                              */
    int32_t max_rounds;          /* 32; >= 0                                                                     */
    int32_t fit_rounds;          /* rounds of the fit after every accepted round: 0 (no fit); >= 0               */
    int32_t reserved;            /* 0                                                                            */
} pagan_anc_nni_opts;
typedef struct pagan_anc_nni_info {
    int32_t status;              /* PAGAN_ANC_NNI_* (pagan_anc_nni_gains: 0)                                     */
    int32_t rounds;              /* gain evaluations made                                                        */
    int32_t up_passes;           /* up passes over the whole alignment, the fit's included                       */
    int32_t chunks;              /* column chunks of one pass                                                    */
    int32_t data_type, states;   /* as pagan_anc_info                                                            */
    int32_t candidates;          /* of the last evaluation's tree                                                */
    int32_t swaps;               /* swaps applied                                                                */
    int64_t columns, chunk_cols;
    int64_t device_bytes;        /* what the call allocated on the device                                        */
    double  loglik_start, loglik_end;
    double  encode_ms, up_ms, down_ms, nni_ms, fold_ms;      /* device time of the stages, summed over the call  */
    double  fit_ms;              /* device time of the fit's branch sums and their fold                          */
    double  total_ms;            /* host wall time of the call                                                   */
} pagan_anc_nni_info;
typedef struct pagan_anc_nni_swap {
    int32_t round;               /* the round that applied it, from 0                                            */
    int32_t node;                /* c, in that round's ids                                                       */
    int32_t k;                   /* 1 or 2                                                                       */
    int32_t joint;               /* 1: applied together with the round's other swaps; 0: alone, after those lowered the loglik */
    double  gain;
} pagan_anc_nni_swap;
/* One evaluation on the device, by internal node (row k: node n + k): kind [n-1] (0 no candidate, 1 ordinary, 2 the root edge);
 * M, gain [(n-1) * 2] and E, degenerate [(n-1) * 2] at [2 k] for arrangement 1 and [2 k + 1] for arrangement 2 -- (0.5, 1), gain 0
 * and 0 where there is no candidate; loglik as pagan_anc_reconstruct's.  Any output may be NULL.  info: rounds 1, up_passes 1.  */
int     pagan_anc_nni_gains(int32_t n_leaves, const int32_t *left, const int32_t *right, const double *branch,
                            const char *const *rows, int32_t data_type, const float *base_freq, int32_t *kind, double *M,
                            int64_t *E, double *gain, int64_t *degenerate, double *loglik, pagan_anc_nni_info *info);
/* Host only.  The swap k (1 or 2) at the candidate `node`, then the renumbering: left_out, right_out [n-1], branch_out [2n-1],
 * perm [2n-1] (may be NULL).  PAGAN_E_TREE as pagan_anc_check_tree; PAGAN_E_ARG for a node without a candidate or another k.   */
int     pagan_anc_nni_apply(int32_t n_leaves, const int32_t *left, const int32_t *right, const double *branch, int32_t node,
                            int32_t k, int32_t *left_out, int32_t *right_out, double *branch_out, int32_t *perm);
/* Host only.  The selection above from gain, degenerate [(n-1) * 2]: nodes_out, k_out [n-1] in the order taken; returns how many,
 * or PAGAN_E_ARG (a null array, min_gain negative or not a number), PAGAN_E_TREE.                                              */
int     pagan_anc_nni_select(int32_t n_leaves, const int32_t *left, const int32_t *right, const double *gain,
                             const int64_t *degenerate, double min_gain, int32_t *nodes_out, int32_t *k_out);
/* The search.  opts NULL: the defaults; PAGAN_E_ARG for a value outside the ranges above.  left_out, right_out [n-1], branch_out
 * [2n-1]: the final tree.  loglik_hist [hist_cap] (may be NULL): the accepted logliks, the start first; the call returns how many
 * there are (accepted rounds + 1; only the first hist_cap are written), or a negative code.  swaps [swap_cap] (may be NULL): the
 * swaps applied, in order; *n_swaps how many there are (only the first swap_cap are written).                                  */
int     pagan_anc_nni_search(int32_t n_leaves, const int32_t *left, const int32_t *right, const double *branch,
                             const char *const *rows, int32_t data_type, const float *base_freq, const pagan_anc_nni_opts *opts,
                             int32_t *left_out, int32_t *right_out, double *branch_out, double *loglik_hist, int32_t hist_cap,
                             pagan_anc_nni_swap *swaps, int32_t swap_cap, int32_t *n_swaps, pagan_anc_nni_info *info);
/* Host only.  Device bytes of a pagan_anc_nni_search or pagan_anc_nni_gains call, under pagan_anc_fit_predict_bytes' contract. */
int64_t pagan_anc_nni_predict_bytes(int32_t n_leaves, int64_t columns, int32_t data_type, int64_t chunk_cols);
/* The search over a finished walk, from its tree and the lengths it aligned under, as pagan_msa_fit_branches takes them.
 * newick_out: the tree found under the walk's names, lengths %.17g; returns the bytes the string needs with its NUL (> cap: the
 * string was not written), or a negative code.  The walk itself is not changed.  PAGAN_E_ARG before the rows exist.            */
int64_t pagan_msa_search_tree(const pagan_msa *m, const pagan_anc_nni_opts *opts, char *newick_out, int64_t cap,
                              pagan_anc_nni_info *info);

/* ---- neighbour joining: the join loop on the device, the rooting and the printing on the host -------------------------
 * (csrc/dp_nj.hip, csrc/host_nj.cpp; DESIGN.md "Neighbour joining").  The alternative to pagan_guide_upgma for lineages that do
 * not keep a molecular clock.  The reference takes such trees from external programs (bppdist method=bionj, raxml, fasttree);
 * none of that is restated.  Every operation below is an fp64 +, -, *, / in the order written, never contracted, so that a
 * second reading reproduces every byte (tests/pycheck_nj.py).
 *
 * Input: pagan_guide_upgma's -- dist [n * n] read at [i * n + j] for i < j, finite and >= 0, names by the same rules;
 * 2 <= n <= PAGAN_NJ_MAX_SEQS (the resident fp64 matrix is then 2 GiB).  Anything else: PAGAN_E_ARG before anything is allocated.
 * Clusters: the leaves are clusters 0 .. n-1, the cluster join t = 0, 1, ... makes is n + t; r, the number of active clusters,
 * starts at n; d(a, a) = 0.
 * Row sums: R_i = sum_k d(i, k) in one fixed order: x[l] = sum_q d(i, 64 q + l), l = 0..63, from +0 with q ascending (the diagonal
 * and indices >= n contribute the exact 0); then for s = 32, 16, 8, 4, 2, 1 in turn x[l] = x[l] + x[l + s] for all l < s;
 * R_i = x[0].  After that R is carried forward and never summed again.
 * A join, while r > 3: for active a, b with id a < id b, Q(a, b) = ((double)(r - 2) * d(a, b) - R_a) - R_b.  The pair of smallest Q
 * is joined (ties: the lowest first id, then the lowest second id).  With i < j the joined ids and u = n + t:
 *   len_i = d(i,j) / 2 + (R_i - R_j) / (2 * (double)(r - 2)),  len_j = d(i,j) - len_i   (raw: either may be negative);
 *   for every other active k: d(u,k) = ((d(i,k) + d(j,k)) - d(i,j)) / 2,  R_k = ((R_k - d(i,k)) - d(j,k)) + d(u,k);
 *   R_u = ((R_i + R_j) - (double)r * d(i,j)) / 2;  r decreases by one.
 * The join record is (i, j, len_i, len_j).
 * The star, at r = 3 (n >= 3), a < b < c the remaining ids: len_a = ((d(a,b) + d(a,c)) - d(b,c)) / 2,
 * len_b = ((d(a,b) + d(b,c)) - d(a,c)) / 2, len_c = ((d(a,c) + d(b,c)) - d(a,b)) / 2, raw as well.  All three Q are equal at
 * r = 3, so the star is never a join; the star node's id is 2 n - 3.  n = 2: no join and no star -- star_ids = {0, 1, -1},
 * star_len = {d / 2, d / 2, 0}, and the tree is (name0:d/2,name1:d/2);
 * Rooting (host only; every length first clamped to max(0, len), as UPGMA's are; a length that is not finite: PAGAN_E_ARG):
 *   the tree hangs from the star node; low(v) is the smallest leaf index below v; a node's children are taken in ascending low;
 *   far(leaf) = 0; for an internal v every child c offers far(c) + len(c), far(v) is the largest offer (a later child replaces an
 *   earlier one only when strictly larger), the second largest offer is taken by the same rule among the other children, and
 *   span(v) is the sum of the two.  The top node is the internal v of largest span, over the internal nodes in id order, a later
 *   one winning only when strictly larger; half = span / 2.  From the top node descend along the child of the largest offer while
 *   far(c) > half: the first c with far(c) <= half carries the root on the edge above it, below = min(max(half - far(c), 0), len(c))
 *   on c's side and above = len(c) - below on the other; the rest of the tree is hung again from that point.  The star node
 *   stays in the tree as an ordinary binary node (two children and the edge above it), also where above = 0 puts the root on it.
 *   Printed as a rooted binary tree: the left child of every node is the one of smaller low; lengths %.17g.
 *
 * Device (pagan_nj_joins, pagan_nj_tree): the symmetric matrix is resident, rows contiguous; the active clusters are kept in the
 * slots 0 .. r-1 (a join puts the new cluster in the lower of the pair's slots and the cluster of slot r-1 in the other).  A join
 * is three dependent launches on one stream -- scan (a wave a row: the row's best (Q, lower id, higher id) over the slots after
 * it), pick (one workgroup: the best row, the join record) and merge (a thread a slot: the new row and column, R) -- and all
 * 3 (n - 3) of them are enqueued without waiting; the host synchronises once and downloads the log once.  One allocation a call.
 * The caller's current device, left current; without a device PAGAN_E_NODEVICE for every n (there is no host path for the join
 * loop); PAGAN_E_NOMEM / PAGAN_E_INTERNAL for a HIP error.  Device time: loop_ms is always measured, by two events; an event
 * between any two launches costs about what a launch costs, so scan_ms, pick_ms and merge_ms are measured only with
 * PAGAN_NJ_EVENTS=1 in the environment and are 0 otherwise.                                                                   */
#define PAGAN_NJ_MAX_SEQS 16384
typedef struct pagan_nj_info {
    int32_t n;                   /* clusters at the start                                                        */
    int32_t joins;               /* n - 3 (0 for n = 2)                                                          */
    int32_t launches;            /* kernels enqueued: the row sums and three a join                              */
    int32_t reserved;            /* 0                                                                            */
    int64_t device_bytes;        /* what the call allocated on the device                                        */
    int64_t scan_entries;        /* matrix entries the scans read, summed over the joins                         */
    double  scan_ms, pick_ms, merge_ms;  /* device time of the stages, summed over the joins (PAGAN_NJ_EVENTS=1: an event
                                    between any two launches; no launch waits for the host), 0 otherwise         */
    double  loop_ms;             /* device time from the first scan to the last merge, two events                */
    double  root_ms;             /* host time of pagan_nj_newick (pagan_nj_tree), 0 otherwise                    */
} pagan_nj_info;
/* The device half.  join_ids, join_len [(n - 3) * 2]: join t's (i, j) and (len_i, len_j) at [2 t], [2 t + 1] (may be NULL where
 * n <= 3); star_ids, star_len [3] as defined above.  info may be NULL.                                                        */
int     pagan_nj_joins(int32_t n, const double *dist, int32_t *join_ids, double *join_len, int32_t star_ids[3], double star_len[3],
                       pagan_nj_info *info);
/* Host only: clamps, roots and prints what pagan_nj_joins returned.  PAGAN_E_ARG also for joins that are no tree (an id that is
 * not active at its join, i >= j, star ids that are not the three clusters left).  Returns what pagan_guide_upgma returns, under
 * the same contract.                                                                                                          */
int64_t pagan_nj_newick(int32_t n, const char *const *names, const int32_t *join_ids, const double *join_len,
                        const int32_t star_ids[3], const double star_len[3], char *newick_out, int64_t cap);
/* pagan_nj_joins, then pagan_nj_newick.  Returns as pagan_nj_newick. */
int64_t pagan_nj_tree(int32_t n, const char *const *names, const double *dist, char *newick_out, int64_t cap, pagan_nj_info *info);
/* Host only, exact: the device bytes a pagan_nj_joins call allocates for n clusters.  PAGAN_E_ARG beyond the limits. */
int64_t pagan_nj_predict_bytes(int32_t n);

#ifdef __cplusplus
}
#endif
#endif /* PAGAN_HOST_H */
