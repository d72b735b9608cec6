"""ctypes front end of include/pagan_host.h: the host-side guide-tree walk (Node mirror), the
host graph builder (Sequence / build_ancestral_sequence mirror), anchors and the DNA model.
All of it lives in libpagan_dp.so; the DP itself always runs on the GPU."""
import ctypes as C

import numpy as np

from . import Handle, PaganError, abi, check, lib  # noqa: F401  (PaganError: what check raises, for callers of this module)
from . import sample_uniforms, sample_uniforms_path  # noqa: F401  (the numbers the walk samples a node's paths with)
from .abi import (_dp, _f32p, _f64p, _fp, _i32p, _i64p, _ip, _u8p, cint, cp, cpp, f32, f64, gp, i32, i64, jp, mpp, rp, struct_dict, u32,
                  vp, vpp)

PAGAN_E_TREE = -20
PAGAN_E_MEMCAP = -21
DNA_FULL = "ACGTRYMKWSBDHVN"


class CMsaOpts(C.Structure):
    _fields_ = [("use_anchors", C.c_int32), ("anchors_offset", C.c_int32), ("prefix_hit_length", C.c_int32),
                ("hit_trim", C.c_int32), ("dp_flags", C.c_uint32), ("leaf_flags", C.c_int32),
                ("keep_all_edges", C.c_int32), ("n_devices", C.c_int32), ("first_device", C.c_int32),
                ("host_threads", C.c_int32), ("truncate_branches", C.c_float), ("device_mem_budget", C.c_int64),
                ("data_type", C.c_int32), ("pileup_rates", C.c_int32), ("anchor_mode", C.c_int32),
                ("overlap_total", C.c_int32), ("overlap_partly", C.c_int32), ("force_gap", C.c_int32),
                ("force_gap_threshold", C.c_int32), ("force_gap_wide", C.c_int32), ("mostcommon", C.c_int32),
                ("full_probability", C.c_int32), ("sample_path", C.c_int32), ("sample_seed", C.c_uint64)]


class CNodeInfo(C.Structure):
    _fields_ = [("node", C.c_int32), ("left", C.c_int32), ("right", C.c_int32), ("level", C.c_int32),
                ("left_sites", C.c_int32), ("right_sites", C.c_int32), ("sites", C.c_int32), ("n_hits", C.c_int32),
                ("cells", C.c_int64), ("dist", C.c_double), ("score", C.c_double), ("status", C.c_int32),
                ("n_forced_gaps", C.c_int32)]


class CTiming(C.Structure):
    _fields_ = [(k, C.c_double) for k in ("total_s", "model_s", "anchors_s", "dp_wall_s", "dp_fill_dev_s",
                                           "dp_trace_dev_s", "build_s")]


# pagan_batch_fn (include/pagan_host.h): the test seam's callback type
BATCH_FN = C.CFUNCTYPE(C.c_int, C.c_int32, C.POINTER(abi.CJob), C.POINTER(abi.COpts), C.POINTER(abi.CResult), C.c_void_p)


class CPileupOpts(C.Structure):
    _fields_ = [("leaf_flags", C.c_int32), ("dp_flags", C.c_uint32), ("query_distance", C.c_float), ("min_overlap", C.c_float),
                ("min_identity", C.c_float), ("use_anchors", C.c_int32), ("anchors_offset", C.c_int32),
                ("prefix_hit_length", C.c_int32), ("hit_trim", C.c_int32), ("device", C.c_int32)]


class CPileupStep(C.Structure):
    _fields_ = [("read", C.c_int32), ("accepted", C.c_int32), ("overlap", C.c_float), ("identity", C.c_float),
                ("aligned", C.c_int32), ("matched", C.c_int32), ("read_length", C.c_int32), ("left_sites", C.c_int32),
                ("right_sites", C.c_int32), ("status", C.c_int32), ("n_cols", C.c_int32), ("score", C.c_double),
                ("cells", C.c_int64)]


class CGuideInfo(C.Structure):
    _fields_ = [("k", C.c_int32), ("data_type", C.c_int32), ("pair_chunk", C.c_int32), ("waves_per_pair", C.c_int32),
                ("positions", C.c_int64), ("entries", C.c_int64), ("pairs", C.c_int64), ("device_bytes", C.c_int64),
                ("pack_ms", C.c_double), ("sort_ms", C.c_double), ("compress_ms", C.c_double), ("pairs_ms", C.c_double),
                ("upgma_ms", C.c_double)]


class CAlnInfo(C.Structure):
    _fields_ = [("data_type", C.c_int32), ("planes", C.c_int32), ("tile", C.c_int32), ("col_splits", C.c_int32),
                ("columns", C.c_int64), ("words", C.c_int64), ("pairs", C.c_int64), ("device_bytes", C.c_int64),
                ("pack_ms", C.c_double), ("pairs_ms", C.c_double), ("upgma_ms", C.c_double)]


class CAncInfo(C.Structure):
    _fields_ = [("data_type", C.c_int32), ("states", C.c_int32), ("chunks", C.c_int32), ("matrices", C.c_int32),
                ("columns", C.c_int64), ("chunk_cols", C.c_int64), ("device_bytes", C.c_int64),
                ("encode_ms", C.c_double), ("up_ms", C.c_double), ("down_ms", C.c_double)]


class CAncFitOpts(C.Structure):
    _fields_ = [("t_min", C.c_double), ("t_max", C.c_double), ("tol", C.c_double), ("max_rounds", C.c_int32), ("reserved", C.c_int32)]


class CAncFitInfo(C.Structure):
    _fields_ = [("status", C.c_int32), ("rounds", C.c_int32), ("up_passes", C.c_int32), ("chunks", C.c_int32),
                ("data_type", C.c_int32), ("states", C.c_int32), ("columns", C.c_int64), ("chunk_cols", C.c_int64),
                ("device_bytes", C.c_int64), ("loglik_start", C.c_double), ("loglik_end", C.c_double),
                ("encode_ms", C.c_double), ("up_ms", C.c_double), ("down_ms", C.c_double), ("branch_ms", C.c_double),
                ("fold_ms", C.c_double), ("total_ms", C.c_double)]


class CAncNniOpts(C.Structure):
    _fields_ = [("min_gain", C.c_double), ("t_min", C.c_double), ("t_max", C.c_double), ("tol", C.c_double),
                ("max_rounds", C.c_int32), ("fit_rounds", C.c_int32), ("reserved", C.c_int32)]


class CAncNniInfo(C.Structure):
    _fields_ = [("status", C.c_int32), ("rounds", C.c_int32), ("up_passes", C.c_int32), ("chunks", C.c_int32),
                ("data_type", C.c_int32), ("states", C.c_int32), ("candidates", C.c_int32), ("swaps", C.c_int32),
                ("columns", C.c_int64), ("chunk_cols", C.c_int64), ("device_bytes", C.c_int64),
                ("loglik_start", C.c_double), ("loglik_end", C.c_double),
                ("encode_ms", C.c_double), ("up_ms", C.c_double), ("down_ms", C.c_double), ("nni_ms", C.c_double),
                ("fold_ms", C.c_double), ("fit_ms", C.c_double), ("total_ms", C.c_double)]


class CAncNniSwap(C.Structure):
    _fields_ = [("round", C.c_int32), ("node", C.c_int32), ("k", C.c_int32), ("joint", C.c_int32), ("gain", C.c_double)]


class CNjInfo(C.Structure):
    _fields_ = [("n", C.c_int32), ("joins", C.c_int32), ("launches", C.c_int32), ("reserved", C.c_int32),
                ("device_bytes", C.c_int64), ("scan_entries", C.c_int64), ("scan_ms", C.c_double), ("pick_ms", C.c_double),
                ("merge_ms", C.c_double), ("loop_ms", C.c_double), ("root_ms", C.c_double)]


GUIDE_MAX_SEQS = 65536
NJ_MAX_SEQS = 16384
TREE_METHODS = ("upgma", "nj")
GUIDE_PAIR_CHUNK = 64
ALN_TILE = 64
ALN_SPLIT_WORDS = 8

# C struct name -> mirror, for every struct the two headers declare with a body
STRUCTS = dict(abi.STRUCTS, pagan_msa_opts=CMsaOpts, pagan_node_info=CNodeInfo, pagan_msa_timing=CTiming,
               pagan_pileup_opts=CPileupOpts, pagan_pileup_step=CPileupStep, pagan_guide_info=CGuideInfo,
               pagan_aln_info=CAlnInfo, pagan_anc_info=CAncInfo, pagan_anc_fit_opts=CAncFitOpts, pagan_anc_fit_info=CAncFitInfo,
               pagan_anc_nni_opts=CAncNniOpts, pagan_anc_nni_info=CAncNniInfo, pagan_anc_nni_swap=CAncNniSwap, pagan_nj_info=CNjInfo)

# Every entry point of include/pagan_host.h in the header's order: name -> (restype, (argtypes...)).  A new entry point is
# one line here; tests/test_abi_cpu.py holds the table against the header's prototypes.
PROTOTYPES = {
    "pagan_msa_default_opts": (None, (C.POINTER(CMsaOpts),)),
    "pagan_assign_units": (None, (i32, _i64p, i32, _i32p)),
    "pagan_msa_create": (cint, (i32, cpp, cpp, cp, C.POINTER(CMsaOpts), vpp)),
    "pagan_msa_align": (cint, (vp,)),
    "pagan_msa_ready": (cint, (vp, _i32p, i32)),
    "pagan_msa_remaining": (cint, (vp,)),
    "pagan_msa_node_cost": (i64, (vp, i32)),
    "pagan_msa_align_nodes": (cint, (vp, i32, _i32p)),
    "pagan_msa_export_result": (i64, (vp, i32, vp, i64)),
    "pagan_msa_import_result": (cint, (vp, vp, i64)),
    "pagan_msa_finish": (cint, (vp,)),
    "pagan_msa_finish_lazy": (cint, (vp,)),
    "pagan_msa_parents_built": (cint, (vp,)),
    "pagan_msa_data_type": (cint, (vp,)),
    "pagan_msa_node_device": (cint, (vp, i32)),
    "pagan_msa_set_batch_backend": (cint, (vp, BATCH_FN, vp)),
    "pagan_msa_set_sampler": (cint, (vp, i32)),
    "pagan_msa_set_decoder": (cint, (vp, i32, f64)),
    "pagan_msa_set_counts": (cint, (vp, i32)),
    "pagan_msa_node_counts": (cint, (vp, i32, _f64p, _f64p)),
    "pagan_msa_set_indel_model": (cint, (vp, f64, f64, f64, f64)),
    "pagan_fit_indel": (cint, (i32, _f64p, _f64p, _f64p, _f64p)),
    "pagan_msa_n_internal": (cint, (vp,)),
    "pagan_msa_node_info": (cint, (vp, i32, C.POINTER(CNodeInfo))),
    "pagan_msa_node_job": (cint, (vp, i32, jp)),
    "pagan_msa_node_result": (cint, (vp, i32, rp)),
    "pagan_msa_node_fb": (cint, (vp, i32, _f64p)),
    "pagan_msa_node_decode": (cint, (vp, i32, _f64p)),
    "pagan_msa_node_support": (cint, (vp, i32, _f64p)),
    "pagan_msa_node_marginals": (cint, (vp, i32, _f64p, _f64p, _i32p, _f64p, _f64p, _f64p, _i32p, _f64p)),
    "pagan_msa_node_model_prob": (cint, (vp, i32, mpp)),
    "pagan_msa_support_row": (cint, (vp, i32, _f32p)),
    "pagan_msa_timing_get": (cint, (vp, C.POINTER(CTiming))),
    "pagan_msa_alignment_length": (cint, (vp,)),
    "pagan_msa_alignment_row": (cint, (vp, i32, cp)),
    "pagan_msa_write_fasta": (cint, (vp, cp, i32)),
    "pagan_msa_write_fasta_nodes": (cint, (vp, cp, i32, i32)),
    "pagan_msa_node_graph": (vp, (vp, i32)),
    "pagan_msa_destroy": (None, (vp,)),
    "pagan_pileup_default_opts": (None, (C.POINTER(CPileupOpts),)),
    "pagan_pileup_create": (cint, (i32, cpp, cpp, C.POINTER(CPileupOpts), vpp)),
    "pagan_pileup_align": (cint, (vp,)),
    "pagan_pileup_n_steps": (cint, (vp,)),
    "pagan_pileup_step_info": (cint, (vp, i32, C.POINTER(CPileupStep))),
    "pagan_pileup_step_job": (cint, (vp, i32, jp)),
    "pagan_pileup_step_result": (cint, (vp, i32, rp)),
    "pagan_pileup_alignment_length": (cint, (vp,)),
    "pagan_pileup_alignment_row": (cint, (vp, i32, cp)),
    "pagan_pileup_set_batch_backend": (cint, (vp, BATCH_FN, vp)),
    "pagan_pileup_destroy": (None, (vp,)),
    "pagan_hgraph_leaf": (vp, (cp, cp, i32)),
    "pagan_hgraph_leaf_codon": (vp, (cp,)),
    "pagan_hgraph_parent": (vp, (vp, vp, rp, f32, f32, _i32p, i32, i32, i32)),
    "pagan_hgraph_parent_device": (vp, (vp, vp, rp, f32, f32, _i32p, i32, i32, i32, _i32p)),
    "pagan_parents_device_calls": (C.c_longlong, ()),
    "pagan_hgraph_view": (None, (vp, gp)),
    "pagan_hgraph_attrs": (None, (vp, _i32p, _f32p, _i32p, _f32p)),
    "pagan_hgraph_fwd": (None, (vp, _i32p, _i32p)),
    "pagan_hgraph_string": (cint, (vp, i32, cp, cp)),
    "pagan_hgraph_free": (None, (vp,)),
    "pagan_define_tunnel": (cint, (cp, cp, cp, cp, i32, i32, i32, _i32p, _i32p)),
    "pagan_prefix_hits": (cint, (cp, cp, i32, _i32p, i32)),
    "pagan_anchors_device_calls": (C.c_longlong, ()),
    "pagan_prefix_hits_raw": (cint, (cp, cp, i32, i32, _i32p, i32)),
    "pagan_drop_bad_hits": (cint, (_i32p, i32, i32, i32)),
    "pagan_define_tunnel_overlapping": (cint, (_i32p, i32, cp, cp, i32, _i32p, _i32p, _i32p, i32)),
    "pagan_force_gap": (cint, (_i32p, _i32p, i32, _i32p, i32, i32, i32, i32)),
    "pagan_dna_model": (cint, (_f32p, f64, _f32p, _f32p, _i32p)),
    "pagan_protein_model": (cint, (f64, _f32p, _f32p, _i32p)),
    "pagan_codon_model": (cint, (f64, _f32p, _f32p, _i32p)),
    "pagan_codon_alphabet": (cint, (cp, _i32p)),
    "pagan_codon_translate": (cint, (cp, cp)),
    "pagan_codon_states": (cint, (cp, _i32p)),
    "pagan_model_prob_table": (cint, (i32, _f32p, f64, _f32p, _f32p)),
    "pagan_model_alphabets": (cint, (i32, cp, cp)),
    "pagan_eigen_qrev": (cint, (_f64p, _f64p, i32, _f64p, _f64p, _f64p)),
    "pagan_guide_distances": (cint, (i32, cpp, i32, i32, _i64p, _i64p, _f64p, C.POINTER(CGuideInfo))),
    "pagan_guide_tree": (i64, (i32, cpp, cpp, i32, i32, cp, i64, C.POINTER(CGuideInfo))),
    "pagan_guide_kmer_length": (cint, (i32, i64)),
    "pagan_guide_distance_of": (f64, (i64, i64, i32, i32)),
    "pagan_guide_upgma": (i64, (i32, cpp, _f64p, cp, i64)),
    "pagan_guide_predict_bytes": (i64, (i32, i64)),
    "pagan_aln_distances": (cint, (i32, cpp, i32, _i64p, _i64p, _f64p, C.POINTER(CAlnInfo))),
    "pagan_aln_tree": (i64, (i32, cpp, cpp, i32, cp, i64, C.POINTER(CAlnInfo))),
    "pagan_aln_predict_bytes": (i64, (i32, i64)),
    "pagan_msa_alignment_tree": (i64, (vp, cp, i64, C.POINTER(CAlnInfo))),
    "pagan_anc_pmatrix": (cint, (i32, _f32p, f64, _f64p, _f64p)),
    "pagan_anc_rate_matrix": (cint, (i32, _f32p, _f64p, _f64p)),
    "pagan_anc_encode_row": (i64, (i32, cp, _u8p)),
    "pagan_anc_check_tree": (cint, (i32, _i32p, _i32p, _f64p)),
    "pagan_anc_predict_bytes": (i64, (i32, i64, i32, i64)),
    "pagan_anc_reconstruct": (cint, (i32, _i32p, _i32p, _f64p, cpp, i32, _f32p, u32, i32, _i32p, _f64p, _i32p, _f64p, _f64p, _u8p,
                                     _f32p, _u8p, _f64p, C.POINTER(CAncInfo))),
    "pagan_msa_ancestral": (cint, (vp, u32, _f64p, _f64p, C.POINTER(CAncInfo))),
    "pagan_msa_ancestral_row": (cint, (vp, i32, cp)),
    "pagan_msa_ancestral_support": (cint, (vp, i32, _f32p)),
    "pagan_msa_write_fasta_ancestral": (cint, (vp, cp, i32)),
    "pagan_msa_ancestral_best": (cint, (vp, C.POINTER(_u8p), C.POINTER(_f32p))),
    "pagan_anc_pmatrix_deriv": (cint, (i32, _f32p, f64, i32, _f64p)),
    "pagan_anc_branch_step": (f64, (f64, f64, f64, f64, f64)),
    "pagan_anc_branch_derivs": (cint, (i32, _i32p, _i32p, _f64p, cpp, i32, _f32p, _f64p, _f64p, _i64p, _f64p, C.POINTER(CAncFitInfo))),
    "pagan_anc_fit_branches": (cint, (i32, _i32p, _i32p, _f64p, cpp, i32, _f32p, C.POINTER(CAncFitOpts), _f64p, _f64p, i32, C.POINTER(CAncFitInfo))),
    "pagan_anc_fit_predict_bytes": (i64, (i32, i64, i32, i64)),
    "pagan_msa_fit_branches": (i64, (vp, C.POINTER(CAncFitOpts), _f64p, cp, i64, C.POINTER(CAncFitInfo))),
    "pagan_anc_nni_gains": (cint, (i32, _i32p, _i32p, _f64p, cpp, i32, _f32p, _i32p, _f64p, _i64p, _f64p, _i64p, _f64p, C.POINTER(CAncNniInfo))),
    "pagan_anc_nni_apply": (cint, (i32, _i32p, _i32p, _f64p, i32, i32, _i32p, _i32p, _f64p, _i32p)),
    "pagan_anc_nni_select": (cint, (i32, _i32p, _i32p, _f64p, _i64p, f64, _i32p, _i32p)),
    "pagan_anc_nni_search": (cint, (i32, _i32p, _i32p, _f64p, cpp, i32, _f32p, C.POINTER(CAncNniOpts), _i32p, _i32p, _f64p, _f64p, i32,
                                    C.POINTER(CAncNniSwap), i32, _i32p, C.POINTER(CAncNniInfo))),
    "pagan_anc_nni_predict_bytes": (i64, (i32, i64, i32, i64)),
    "pagan_msa_search_tree": (i64, (vp, C.POINTER(CAncNniOpts), cp, i64, C.POINTER(CAncNniInfo))),
    "pagan_nj_joins": (cint, (i32, _f64p, _i32p, _f64p, _i32p, _f64p, C.POINTER(CNjInfo))),
    "pagan_nj_newick": (i64, (i32, cpp, _i32p, _f64p, _i32p, _f64p, cp, i64)),
    "pagan_nj_tree": (i64, (i32, cpp, _f64p, cp, i64, C.POINTER(CNjInfo))),
    "pagan_nj_predict_bytes": (i64, (i32,)),
}
HOST_EXPORTED = list(PROTOTYPES)


def _lib():
    """The loaded library: every entry point of both headers is declared from the moment lib() loads it."""
    return lib()


def _graph_from_view(v):
    """Copies a borrowed pagan_graph view into an abi.Graph."""
    ns = v.n_sites
    off = np.ctypeslib.as_array(v.bwd_off, shape=(ns + 1,)).copy()
    nb = int(off[-1])
    if nb:
        src = np.ctypeslib.as_array(v.bwd_src, shape=(nb,)).copy()
        lw = np.ctypeslib.as_array(v.bwd_logw, shape=(nb,)).copy()
        eid = np.ctypeslib.as_array(v.bwd_eid, shape=(nb,)).copy()
    else:
        src, lw, eid = np.zeros(0, np.int32), np.zeros(0, np.float32), np.zeros(0, np.int32)
    return abi.Graph(np.ctypeslib.as_array(v.state, shape=(ns,)).copy(), off, src, lw, eid, n_edges=v.n_edges)


def _result_view(result):
    """(a pagan_result over an abi.Result's columns and used edges, the arrays it points into)."""
    keep = [np.ascontiguousarray(a, np.int32) for a in (result.cols, result.left_used, result.right_used)]
    r = abi.CResult()
    r.n_cols, r.cols = int(keep[0].shape[0]), C.cast(_ip(keep[0]), abi.colp)
    r.n_left_used, r.left_used = int(keep[1].shape[0]), _ip(keep[1])
    r.n_right_used, r.right_used = int(keep[2].shape[0]), _ip(keep[2])
    return r, keep


class HGraph(Handle):
    """Host sequence graph (leaf or parent).  `owned=False` for graphs borrowed from an Msa, which `keep` keeps alive."""
    _destroy = "pagan_hgraph_free"
    h = property(lambda self: self._h)

    def __init__(self, handle, owned=True, keep=None):
        self._h, self.owned, self._keep = handle, owned, keep

    @classmethod
    def leaf(cls, seq, alphabet=DNA_FULL, flags=0):
        return cls(_lib().pagan_hgraph_leaf(seq.encode(), alphabet.encode(), flags))

    @classmethod
    def codon_leaf(cls, nucleotides):
        """One site per triplet (Sequence::create_codon_sequence)."""
        return cls(_lib().pagan_hgraph_leaf_codon(nucleotides.encode()))

    @classmethod
    def parent(cls, left, right, result, lbl, rbl, parsimony, char_as, flags=0):
        """result: abi.Result (columns + used edges) of aligning left and right."""
        r, _keep = _result_view(result)
        pars = np.ascontiguousarray(parsimony, np.int32)
        S = int(round(pars.size ** 0.5))
        return cls(_lib().pagan_hgraph_parent(left.h, right.h, C.byref(r), lbl, rbl, _ip(pars), S, char_as, flags))

    @classmethod
    def parent_device(cls, left, right, result, lbl, rbl, parsimony, char_as, flags=0):
        """The same parent built on the current HIP device (csrc/dp_parent.hip).  Raises without a device: there is no
        host graph in its place.  The returned graph carries `.build_info` = (runs of skipped sites, rounds of the boundary
        pass, deleted sites, weights outside the log table, log weights corrected by the host)."""
        r, _keep = _result_view(result)
        pars = np.ascontiguousarray(parsimony, np.int32)
        S = int(round(pars.size ** 0.5))
        info = np.zeros(8, np.int32)
        h = _lib().pagan_hgraph_parent_device(left.h, right.h, C.byref(r), lbl, rbl, _ip(pars), S, char_as, flags, _ip(info))
        if not h:
            raise RuntimeError("pagan_hgraph_parent_device failed: no HIP device, or a HIP error")
        g = cls(h)
        g.build_info = tuple(int(x) for x in info[:5])
        return g

    def flatten(self):
        v = abi.CGraph()
        _lib().pagan_hgraph_view(self.h, C.byref(v))
        return _graph_from_view(v)

    def attrs(self):
        v = abi.CGraph()
        L = _lib()
        L.pagan_hgraph_view(self.h, C.byref(v))
        ns, ne = v.n_sites, v.n_edges
        sa = np.zeros((ns, 8), np.int32)
        sd = np.zeros(ns, np.float32)
        ea = np.zeros((max(ne, 1), 6), np.int32)
        ef = np.zeros((max(ne, 1), 3), np.float32)
        L.pagan_hgraph_attrs(self.h, _ip(sa), _fp(sd), _ip(ea), _fp(ef))
        return sa, sd, ea[:ne], ef[:ne]

    def fwd(self):
        v = abi.CGraph()
        L = _lib()
        L.pagan_hgraph_view(self.h, C.byref(v))
        off = np.zeros(v.n_sites + 1, np.int32)
        eid = np.zeros(max(v.n_edges, 1), np.int32)
        L.pagan_hgraph_fwd(self.h, _ip(off), _ip(eid))
        return off, eid[:off[-1]]

    def string(self, with_gaps, alphabet=DNA_FULL):
        v = abi.CGraph()
        L = _lib()
        L.pagan_hgraph_view(self.h, C.byref(v))
        buf = C.create_string_buffer(3 * v.n_sites + 1)              # codon graphs write three characters per site
        n = L.pagan_hgraph_string(self.h, 1 if with_gaps else 0, alphabet.encode(), buf)
        return buf.raw[:n].decode()


def assign_units(costs, n_workers):
    """owner[k] for every unit: largest first, least-loaded worker (pagan_assign_units)."""
    c = np.ascontiguousarray(costs, np.int64)
    owner = np.zeros(c.shape[0], np.int32)
    _lib().pagan_assign_units(int(c.shape[0]), c.ctypes.data_as(_i64p), int(n_workers), _ip(owner))
    return owner


def define_tunnel(s1, s2, g1, g2, prefix_hit_length=30, hit_trim=5, offset=15):
    up = np.zeros(len(g1) + 1, np.int32)
    lo = np.zeros(len(g1) + 1, np.int32)
    n = _lib().pagan_define_tunnel(s1.encode(), s2.encode(), g1.encode(), g2.encode(), prefix_hit_length, hit_trim,
                                   offset, _ip(up), _ip(lo))
    return abi.Band(up, lo), n


def prefix_hits(s1, s2, min_length=30):
    """Find_anchors::find_long_substrings: [n, 4] int32 rows (start 1, start 2, length, score)."""
    cap = max(len(s1), 1)
    out = np.zeros((cap, 4), np.int32)
    n = _lib().pagan_prefix_hits(s1.encode(), s2.encode(), min_length, _ip(out), cap)
    return out[:n].copy()


def prefix_hits_raw(s1, s2, min_length=30, device=False):
    """The list prefix_hits() starts from, before its sort by length and its overlap filter: the adjacent cross-string pairs of
    the suffix array in suffix-array order, [n, 3] int32 rows (start 1, start 2, length).  s1, s2: bytes, or str read as
    latin-1 (no NUL).  device=True: the device's finder whatever the lengths (pagan_prefix_hits_raw, where = 1); raises
    RuntimeError with the library's code where it declines."""
    s1 = s1.encode("latin-1") if isinstance(s1, str) else bytes(s1)
    s2 = s2.encode("latin-1") if isinstance(s2, str) else bytes(s2)
    if b"\0" in s1 or b"\0" in s2:
        raise ValueError("NUL ends a C string")
    cap = len(s1) + len(s2) + 1
    out = np.zeros((cap, 3), np.int32)
    n = _lib().pagan_prefix_hits_raw(s1, s2, min_length, 1 if device else 0, _ip(out), cap)
    if n < 0:
        raise RuntimeError("pagan_prefix_hits_raw: error %d" % n)
    return out[:n].copy()


def anchors_device_calls():
    """how often the prefix-anchor finder has run on the device in this process"""
    return int(_lib().pagan_anchors_device_calls())


def drop_bad_hits(hits, thr_total=50, thr_partly=400):
    h = np.ascontiguousarray(hits, np.int32).reshape(-1, 4).copy()
    n = _lib().pagan_drop_bad_hits(_ip(h), int(h.shape[0]), thr_total, thr_partly)
    return h[:n].copy()


def define_tunnel_overlapping(hits, g1, g2, width=15):
    """(Band, blocks[n, 4]) from possibly overlapping hits (define_tunnel_with_overlapping_hits)."""
    h = np.ascontiguousarray(hits, np.int32).reshape(-1, 4)
    up = np.zeros(len(g1) + 1, np.int32)
    lo = np.zeros(len(g1) + 1, np.int32)
    cap = len(g1) + 2
    blocks = np.zeros((cap, 4), np.int32)
    n = check(_lib().pagan_define_tunnel_overlapping(_ip(h), int(h.shape[0]), g1.encode(), g2.encode(), width, _ip(up), _ip(lo),
                                                     _ip(blocks), cap), "pagan_define_tunnel_overlapping")
    return abi.Band(up, lo), blocks[:n].copy()


def force_gap(band, blocks, threshold=40000, width=15, wide=False):
    """One round of --force-gap: (replaced?, new Band, remaining blocks)."""
    up, lo = band.upper.copy(), band.lower.copy()
    b = np.ascontiguousarray(blocks, np.int32).reshape(-1, 4)
    done = _lib().pagan_force_gap(_ip(up), _ip(lo), int(up.shape[0]), _ip(b), int(b.shape[0]), threshold, width, 1 if wide else 0)
    return bool(done), abi.Band(up, lo), (b[:-1].copy() if done else b.copy())


def dna_model(base_freq, dist):
    """(abi.Model, parsimony[225]) for a DNA alignment at distance `dist`."""
    bf = np.ascontiguousarray(base_freq, np.float32)
    table = np.zeros(225, np.float32)
    params = np.zeros(4, np.float32)
    pars = np.zeros(225, np.int32)
    check(_lib().pagan_dna_model(_fp(bf), float(dist), _fp(table), _fp(params), _ip(pars)), "pagan_dna_model")
    return abi.Model(table.reshape(15, 15).T, *params), pars


def protein_model(dist):
    """(abi.Model, parsimony[211*211]) for a protein (WAG) alignment at distance `dist`."""
    table = np.zeros(211 * 211, np.float32)
    params = np.zeros(4, np.float32)
    pars = np.zeros(211 * 211, np.int32)
    check(_lib().pagan_protein_model(float(dist), _fp(table), _fp(params), _ip(pars)), "pagan_protein_model")
    return abi.Model(table.reshape(211, 211).T, *params), pars


CODON_STATES = 61 + 1 + 1830


def codon_model(dist):
    """(abi.Model, parsimony[1892*1892]) for a codon alignment (Kosiol & Goldman's empirical model) at distance `dist`."""
    S = CODON_STATES
    table = np.zeros(S * S, np.float32)
    params = np.zeros(4, np.float32)
    pars = np.zeros(S * S, np.int32)
    check(_lib().pagan_codon_model(float(dist), _fp(table), _fp(params), _ip(pars)), "pagan_codon_model")
    return abi.Model(table.reshape(S, S).T, *params), pars


def codon_alphabet():
    """(flat string of three-letter state names -- the first 62 are the leaf codons and NNN --, mostcommon[61*61])"""
    buf = C.create_string_buffer(3 * CODON_STATES + 1)
    mc = np.zeros(61 * 61, np.int32)
    _lib().pagan_codon_alphabet(buf, _ip(mc))
    return buf.value.decode(), mc


def codon_translate(codon_string):
    """One amino-acid letter per triplet (Codon_translation::gapped_DNA_to_protein)."""
    buf = C.create_string_buffer(len(codon_string) // 3 + 2)
    n = check(_lib().pagan_codon_translate(codon_string.encode(), buf), "pagan_codon_translate")
    return buf.raw[:n].decode()


def codon_states(nucleotides):
    out = np.zeros(len(nucleotides) // 3 + 2, np.int32)
    n = check(_lib().pagan_codon_states(nucleotides.encode(), _ip(out)), "pagan_codon_states")
    return out[:n].copy()


def model_prob(data_type, dist, base_freq=None):
    """abi.ModelProb for a distance: the probability-space view (Evol_model::score, gap_open, gap_ext, non_gap)."""
    S = CODON_STATES if data_type == 3 else 211 if data_type == 2 else 15
    score = np.zeros(S * S, np.float32)
    params = np.zeros(3, np.float32)
    bf = np.ascontiguousarray(base_freq if base_freq is not None else [0.25] * 4, np.float32)
    check(_lib().pagan_model_prob_table(int(data_type), _fp(bf), float(dist), _fp(score), _fp(params)), "pagan_model_prob_table")
    return abi.ModelProb(score.reshape(S, S).T, *params)


def fit_indel(dists, trans):
    """pagan_fit_indel (host only): (indel_rate, gap_ext) from the nodes' distances [n] and expected counts [n, 12] -- trans[3 * from
    + to] over X, Y, M, then X-close, Y-close, M-end (a [3, 3] and a [3] array per node are accepted as Msa.node_counts gives them).
    A moment / pseudo-likelihood estimate (include/pagan_host.h), not a maximum-likelihood fit of the model as scored."""
    d = np.ascontiguousarray(dists, np.float64).reshape(-1)
    rows = [np.concatenate([np.asarray(t["trans"], np.float64).reshape(9), np.asarray(t["end"], np.float64).reshape(3)])
            if isinstance(t, dict) else np.asarray(t, np.float64).reshape(12) for t in trans]
    t = np.ascontiguousarray(np.array(rows, np.float64).reshape(-1, 12))
    assert t.shape[0] == d.shape[0]
    rate, ext = C.c_double(), C.c_double()
    check(_lib().pagan_fit_indel(int(d.shape[0]), _dp(d), _dp(t), C.byref(rate), C.byref(ext)), "pagan_fit_indel")
    return rate.value, ext.value


def alphabets(data_type):
    """(leaf alphabet, ancestral alphabet) of a data type: 1 DNA, 2 protein."""
    a, b = C.create_string_buffer(256), C.create_string_buffer(256)
    _lib().pagan_model_alphabets(int(data_type), a, b)
    return a.value.decode(), b.value.decode()


def eigen_qrev(Q, pi):
    """Eigen::eigenQREV as the library restates it: (root, U, V) with Q = U diag(root) V."""
    Q = np.ascontiguousarray(Q, np.float64)
    pi = np.ascontiguousarray(pi, np.float64)
    n = pi.shape[0]
    root, U, V = np.zeros(n), np.zeros((n, n)), np.zeros((n, n))
    check(_lib().pagan_eigen_qrev(_dp(Q), _dp(pi), n, _dp(root), _dp(U), _dp(V)), "pagan_eigen_qrev")
    return root, U, V


def _c_strings(strings):
    return (C.c_char_p * len(strings))(*[s.encode() if isinstance(s, str) else bytes(s) for s in strings])


def guide_kmer_length(data_type, max_len):
    """pagan_guide_kmer_length (host only): the default k for sequences of at most max_len cleaned letters."""
    return check(_lib().pagan_guide_kmer_length(int(data_type), int(max_len)), "pagan_guide_kmer_length")


def guide_distance_of(shared, m, k, data_type):
    """pagan_guide_distance_of (host only): the distance from S, m = min(|n_x|, |n_y|) and k; NaN for arguments outside the domain."""
    return float(_lib().pagan_guide_distance_of(int(shared), int(m), int(k), int(data_type)))


def guide_predict_bytes(n, total_len):
    """pagan_guide_predict_bytes (host only): device bytes guide_distances allocates at most."""
    return check(_lib().pagan_guide_predict_bytes(int(n), int(total_len)), "pagan_guide_predict_bytes")


def guide_distances(seqs, data_type=0, k=0):
    """pagan_guide_distances: (shared [n, n] int64, kmers [n] int64, dist [n, n] float64, info dict) -- the k-mers every pair of
    sequences shares, counted on the current device, and the distances made of them (include/pagan_host.h)."""
    n = len(seqs)
    shared = np.zeros((n, n), np.int64)
    kmers = np.zeros(n, np.int64)
    dist = np.zeros((n, n), np.float64)
    ci = CGuideInfo()
    check(_lib().pagan_guide_distances(n, _c_strings(seqs), int(data_type), int(k), shared.ctypes.data_as(_i64p),
                                       kmers.ctypes.data_as(_i64p), _dp(dist), C.byref(ci)), "pagan_guide_distances")
    return shared, kmers, dist, struct_dict(ci)


def _newick_call(call, what, names):
    cap = sum(len(s) for s in names) + 64 * len(names) + 64        # (a branch prints as at most 24 characters)
    for _ in range(2):
        buf = C.create_string_buffer(cap)
        need = check(call(buf, cap), what)
        if need <= cap:
            return buf.value.decode()
        cap = need
    raise RuntimeError("%s: the string's size changed between two calls" % what)


def _tree_method(method):
    if method not in TREE_METHODS:
        raise ValueError("the tree method is 'upgma' or 'nj'")
    return method == "nj"


def guide_tree(names, seqs, data_type=0, k=0, with_info=False, method="upgma"):
    """pagan_guide_tree: the rooted binary UPGMA tree over guide_distances' matrix as a Newick string (with_info: and the info
    dict), ready for Msa.  method="nj": nj_tree over the same matrix (the info dict: guide_distances', with nj_tree's as "nj")."""
    n = len(names)
    if len(seqs) != n:
        raise ValueError("names and sequences differ in number")
    if _tree_method(method):
        _, _, dist, info = guide_distances(seqs, data_type, k)
        newick, info["nj"] = nj_tree(names, dist, with_info=True)
        return (newick, info) if with_info else newick
    na, sa = _c_strings(names), _c_strings(seqs)
    ci = CGuideInfo()
    L = _lib()
    newick = _newick_call(lambda buf, cap: L.pagan_guide_tree(n, na, sa, int(data_type), int(k), buf, cap, C.byref(ci)),
                          "pagan_guide_tree", names)
    return (newick, struct_dict(ci)) if with_info else newick


def guide_upgma(names, dist):
    """pagan_guide_upgma (host only): the UPGMA tree over a distance matrix [n, n] (its upper triangle is read) as Newick."""
    n = len(names)
    d = np.ascontiguousarray(dist, np.float64)
    if d.shape != (n, n):
        raise ValueError("dist must be [%d, %d]" % (n, n))
    na = _c_strings(names)
    L = _lib()
    return _newick_call(lambda buf, cap: L.pagan_guide_upgma(n, na, _dp(d), buf, cap), "pagan_guide_upgma", names)


def aln_predict_bytes(n, columns):
    """pagan_aln_predict_bytes (host only): device bytes aln_distances allocates at most for n rows of `columns` columns."""
    return check(_lib().pagan_aln_predict_bytes(int(n), int(columns)), "pagan_aln_predict_bytes")


def aln_distances(rows, data_type=0):
    """pagan_aln_distances: (both [n, n] int64, match [n, n] int64, dist [n, n] float64, info dict) -- for every pair of rows of
    an alignment the columns where both hold a letter and those of them where the letters agree, counted on the current device,
    and the distances made of them (include/pagan_host.h)."""
    n = len(rows)
    both = np.zeros((n, n), np.int64)
    match = np.zeros((n, n), np.int64)
    dist = np.zeros((n, n), np.float64)
    ci = CAlnInfo()
    check(_lib().pagan_aln_distances(n, _c_strings(rows), int(data_type), both.ctypes.data_as(_i64p), match.ctypes.data_as(_i64p),
                                     _dp(dist), C.byref(ci)), "pagan_aln_distances")
    return both, match, dist, struct_dict(ci)


def aln_tree(names, rows, data_type=0, with_info=False, method="upgma"):
    """pagan_aln_tree: the rooted binary UPGMA tree over aln_distances' matrix as a Newick string (with_info: and the info dict),
    ready for Msa.  method="nj": nj_tree over the same matrix (the info dict: aln_distances', with nj_tree's as "nj")."""
    n = len(names)
    if len(rows) != n:
        raise ValueError("names and rows differ in number")
    if _tree_method(method):
        _, _, dist, info = aln_distances(rows, data_type)
        newick, info["nj"] = nj_tree(names, dist, with_info=True)
        return (newick, info) if with_info else newick
    na, ra = _c_strings(names), _c_strings(rows)
    ci = CAlnInfo()
    L = _lib()
    newick = _newick_call(lambda buf, cap: L.pagan_aln_tree(n, na, ra, int(data_type), buf, cap, C.byref(ci)), "pagan_aln_tree", names)
    return (newick, struct_dict(ci)) if with_info else newick


def nj_predict_bytes(n):
    """pagan_nj_predict_bytes (host only): the device bytes nj_joins allocates for n clusters, exactly."""
    return check(_lib().pagan_nj_predict_bytes(int(n)), "pagan_nj_predict_bytes")


def _nj_dist(n, dist):
    d = np.ascontiguousarray(dist, np.float64)
    if d.shape != (n, n):
        raise ValueError("dist must be [%d, %d]" % (n, n))
    return d


def nj_joins(dist):
    """pagan_nj_joins: the joins of neighbour joining over a distance matrix [n, n] (its upper triangle is read), made on the
    current device: (join_ids [n - 3, 2] int32, join_len [n - 3, 2] float64, star_ids [3] int32, star_len [3] float64, info dict)
    as include/pagan_host.h defines them; the lengths are raw."""
    n = len(dist)
    d = _nj_dist(n, dist)
    joins = max(n - 3, 0)
    ids, lens = np.zeros((joins, 2), np.int32), np.zeros((joins, 2), np.float64)
    star_ids, star_len = np.zeros(3, np.int32), np.zeros(3, np.float64)
    ci = CNjInfo()
    check(_lib().pagan_nj_joins(n, _dp(d), _ip(ids) if joins else None, _dp(lens) if joins else None, _ip(star_ids), _dp(star_len),
                                C.byref(ci)), "pagan_nj_joins")
    return ids, lens, star_ids, star_len, struct_dict(ci)


def nj_newick(names, join_ids, join_len, star_ids, star_len):
    """pagan_nj_newick (host only): the joins' tree with its lengths clamped at 0, rooted at the midpoint of its longest path and
    printed as a rooted binary Newick string, the left child of every node the one with the smaller lowest leaf."""
    n = len(names)
    joins = max(n - 3, 0)
    ids = np.ascontiguousarray(join_ids, np.int32).reshape(-1)
    lens = np.ascontiguousarray(join_len, np.float64).reshape(-1)
    sid, slen = np.ascontiguousarray(star_ids, np.int32).reshape(-1), np.ascontiguousarray(star_len, np.float64).reshape(-1)
    if len(ids) != 2 * joins or len(lens) != 2 * joins or len(sid) != 3 or len(slen) != 3:
        raise ValueError("%d names take %d joins and a star of three" % (n, joins))
    na = _c_strings(names)
    L = _lib()
    return _newick_call(lambda buf, cap: L.pagan_nj_newick(n, na, _ip(ids) if joins else None, _dp(lens) if joins else None, _ip(sid),
                                                           _dp(slen), buf, cap), "pagan_nj_newick", names)


def nj_tree(names, dist, with_info=False):
    """pagan_nj_tree: nj_newick over nj_joins -- the rooted binary neighbour-joining tree over a distance matrix [n, n] as a
    Newick string (with_info: and the info dict), ready for Msa."""
    n = len(names)
    d = _nj_dist(n, dist)
    na = _c_strings(names)
    ci = CNjInfo()
    L = _lib()
    newick = _newick_call(lambda buf, cap: L.pagan_nj_tree(n, na, _dp(d), buf, cap, C.byref(ci)), "pagan_nj_tree", names)
    return (newick, struct_dict(ci)) if with_info else newick


ANC_STATES = {1: 4, 2: 20, 3: 61}


def _base_freq(base_freq):
    if base_freq is None:
        return None, None
    bf = np.ascontiguousarray(base_freq, np.float32)
    if bf.shape != (4,):
        raise ValueError("base_freq must hold four frequencies")
    return bf, _fp(bf)


def anc_pmatrix(data_type, t, base_freq=None):
    """pagan_anc_pmatrix (host only): (P [S, S], pi [S]) of the walk's substitution model over its core states (S = 4 / 20 / 61
    for data_type 1 / 2 / 3) for branch length t; base_freq (DNA only) as dna_model takes it."""
    S = ANC_STATES.get(int(data_type), 1)
    P, pi = np.zeros((S, S), np.float64), np.zeros(S, np.float64)
    _keep, bfp = _base_freq(base_freq)
    check(_lib().pagan_anc_pmatrix(int(data_type), bfp, float(t), _dp(P), _dp(pi)), "pagan_anc_pmatrix")
    return P, pi


def anc_rate_matrix(data_type, base_freq=None):
    """pagan_anc_rate_matrix (host only): (Q [S, S], pi [S]) -- the rate matrix anc_pmatrix exponentiates, the model's made proper."""
    S = ANC_STATES.get(int(data_type), 1)
    Q, pi = np.zeros((S, S), np.float64), np.zeros(S, np.float64)
    _keep, bfp = _base_freq(base_freq)
    check(_lib().pagan_anc_rate_matrix(int(data_type), bfp, _dp(Q), _dp(pi)), "pagan_anc_rate_matrix")
    return Q, pi


def anc_encode_row(data_type, row):
    """pagan_anc_encode_row (host only): the row's leaf codes (uint8) by the tables the device encodes with -- DNA the state set as
    bits (0: missing data), protein and codon the state (255: missing data)."""
    raw = row.encode() if isinstance(row, str) else bytes(row)
    codes = np.zeros(max(len(raw), 1), np.uint8)
    n = check(_lib().pagan_anc_encode_row(int(data_type), raw, codes.ctypes.data_as(_u8p)), "pagan_anc_encode_row")
    return codes[:n].copy()


def anc_check_tree(left, right, branch):
    """pagan_anc_check_tree (host only): raises PaganError(PAGAN_E_TREE) for a tree the reconstruction would refuse."""
    le, ri = np.ascontiguousarray(left, np.int32), np.ascontiguousarray(right, np.int32)
    br = np.ascontiguousarray(branch, np.float64)
    n = len(le) + 1
    if len(ri) != n - 1 or len(br) != 2 * n - 1:
        raise ValueError("left, right hold n - 1 entries and branch 2 n - 1")
    check(_lib().pagan_anc_check_tree(n, _ip(le), _ip(ri), _dp(br)), "pagan_anc_check_tree")


def anc_predict_bytes(n_leaves, columns, data_type, chunk_cols=0):
    """pagan_anc_predict_bytes (host only): device bytes anc_reconstruct allocates at most."""
    return check(_lib().pagan_anc_predict_bytes(int(n_leaves), int(columns), int(data_type), int(chunk_cols)), "pagan_anc_predict_bytes")


def anc_reconstruct(left, right, branch, rows, data_type=0, base_freq=None, post_nodes=()):
    """pagan_anc_reconstruct: marginal ancestral states of an alignment on its tree, on the current device.  left, right [n - 1]:
    the children of internal node n + k; branch [2 n - 1]: the length above every node.  Returns a dict: col_lik, col_exp,
    col_loglik [L]; loglik; best (uint8), best_p (float32) [n - 1, L]; has_data (uint8) [2 n - 1, L]; post [len(post_nodes), L, S];
    info (include/pagan_host.h)."""
    le, ri = np.ascontiguousarray(left, np.int32), np.ascontiguousarray(right, np.int32)
    br = np.ascontiguousarray(branch, np.float64)
    n = len(rows)
    if len(le) != n - 1 or len(ri) != n - 1 or len(br) != 2 * n - 1:
        raise ValueError("left, right hold n - 1 entries and branch 2 n - 1")
    pn = np.ascontiguousarray(post_nodes, np.int32)
    chars = len(rows[0]) if n else 0
    _keep, bfp = _base_freq(base_freq)
    ci = CAncInfo()
    # the columns are known only once the data type is resolved: size for one character a column, cut afterwards
    col_lik, col_exp, col_loglik = np.zeros(chars, np.float64), np.zeros(chars, np.int32), np.zeros(chars, np.float64)
    loglik = C.c_double(0.0)
    best, best_p = np.zeros((n - 1) * chars, np.uint8), np.zeros((n - 1) * chars, np.float32)
    has = np.zeros((2 * n - 1) * chars, np.uint8)
    post = np.zeros(len(pn) * chars * ANC_STATES[3], np.float64)
    check(_lib().pagan_anc_reconstruct(n, _ip(le), _ip(ri), _dp(br), _c_strings(rows), int(data_type), bfp, 0, len(pn), _ip(pn),
                                       _dp(col_lik), _ip(col_exp), _dp(col_loglik), C.byref(loglik), best.ctypes.data_as(_u8p),
                                       _fp(best_p), has.ctypes.data_as(_u8p), _dp(post), C.byref(ci)), "pagan_anc_reconstruct")
    L, S = int(ci.columns), int(ci.states)
    return {"col_lik": col_lik[:L].copy(), "col_exp": col_exp[:L].copy(), "col_loglik": col_loglik[:L].copy(), "loglik": loglik.value,
            "best": best[:(n - 1) * L].reshape(n - 1, L).copy(), "best_p": best_p[:(n - 1) * L].reshape(n - 1, L).copy(),
            "has_data": has[:(2 * n - 1) * L].reshape(2 * n - 1, L).copy(), "post": post[:len(pn) * L * S].reshape(len(pn), L, S).copy(),
            "info": struct_dict(ci)}


ANC_FIT_CONVERGED, ANC_FIT_MAX_ROUNDS, ANC_FIT_STALLED = 0, 1, 2
ANC_FIT_STATUS = {ANC_FIT_CONVERGED: "converged", ANC_FIT_MAX_ROUNDS: "max_rounds", ANC_FIT_STALLED: "stalled"}


def anc_pmatrix_deriv(data_type, t, order, base_freq=None):
    """pagan_anc_pmatrix_deriv (host only): D_order(t) [S, S], order 1 or 2 -- the eigen sum of anc_pmatrix with root^order in
    every term, not clamped (include/pagan_host.h, "branch lengths by maximum likelihood")."""
    S = ANC_STATES.get(int(data_type), 1)
    D = np.zeros((S, S), np.float64)
    _keep, bfp = _base_freq(base_freq)
    check(_lib().pagan_anc_pmatrix_deriv(int(data_type), bfp, float(t), int(order), _dp(D)), "pagan_anc_pmatrix_deriv")
    return D


def anc_branch_step(t, g1, g2, t_min=1e-6, t_max=10.0):
    """pagan_anc_branch_step (host only): the fit's step rule for one branch."""
    return float(_lib().pagan_anc_branch_step(float(t), float(g1), float(g2), float(t_min), float(t_max)))


def _anc_tree_args(left, right, branch, rows):
    le, ri = np.ascontiguousarray(left, np.int32), np.ascontiguousarray(right, np.int32)
    br = np.ascontiguousarray(branch, np.float64)
    n = len(rows)
    if len(le) != n - 1 or len(ri) != n - 1 or len(br) != 2 * n - 1:
        raise ValueError("left, right hold n - 1 entries and branch 2 n - 1")
    return n, le, ri, br


def _anc_fit_opts(t_min, t_max, tol, max_rounds):
    return CAncFitOpts(float(t_min), float(t_max), float(tol), int(max_rounds), 0)


def _anc_fit_info(ci):
    info = struct_dict(ci)
    info["status"] = ANC_FIT_STATUS.get(info["status"], info["status"])
    return info


def anc_branch_derivs(left, right, branch, rows, data_type=0, base_freq=None):
    """pagan_anc_branch_derivs: one evaluation on the current device.  Returns a dict: g1, g2 (float64), informative (int64)
    [2 n - 1] by node id, the root's entries 0; loglik (anc_reconstruct's); info."""
    n, le, ri, br = _anc_tree_args(left, right, branch, rows)
    _keep, bfp = _base_freq(base_freq)
    g1, g2, inf = np.zeros(2 * n - 1, np.float64), np.zeros(2 * n - 1, np.float64), np.zeros(2 * n - 1, np.int64)
    loglik, ci = C.c_double(0.0), CAncFitInfo()
    check(_lib().pagan_anc_branch_derivs(n, _ip(le), _ip(ri), _dp(br), _c_strings(rows), int(data_type), bfp, _dp(g1), _dp(g2),
                                         inf.ctypes.data_as(_i64p), C.byref(loglik), C.byref(ci)), "pagan_anc_branch_derivs")
    return {"g1": g1, "g2": g2, "informative": inf, "loglik": loglik.value, "info": _anc_fit_info(ci)}


def anc_fit_branches(left, right, branch, rows, data_type=0, base_freq=None, t_min=1e-6, t_max=10.0, tol=1e-6, max_rounds=32):
    """pagan_anc_fit_branches: the branch lengths of largest likelihood for the rows on the tree, from `branch`, on the current
    device.  Returns a dict: branch [2 n - 1] (the root's entry 0), loglik (the accepted log likelihoods, the start first: never
    decreasing), info (status as "converged" / "max_rounds" / "stalled", rounds, up_passes, loglik_start, loglik_end, ...)."""
    n, le, ri, br = _anc_tree_args(left, right, branch, rows)
    _keep, bfp = _base_freq(base_freq)
    o = _anc_fit_opts(t_min, t_max, tol, max_rounds)
    out, hist, ci = np.zeros(2 * n - 1, np.float64), np.zeros(int(max(max_rounds, 0)) + 1, np.float64), CAncFitInfo()
    k = check(_lib().pagan_anc_fit_branches(n, _ip(le), _ip(ri), _dp(br), _c_strings(rows), int(data_type), bfp, C.byref(o), _dp(out),
                                            _dp(hist), len(hist), C.byref(ci)), "pagan_anc_fit_branches")
    return {"branch": out, "loglik": hist[:k].copy(), "info": _anc_fit_info(ci)}


def anc_fit_predict_bytes(n_leaves, columns, data_type, chunk_cols=0):
    """pagan_anc_fit_predict_bytes (host only): device bytes anc_fit_branches or anc_branch_derivs allocates at most."""
    return check(_lib().pagan_anc_fit_predict_bytes(int(n_leaves), int(columns), int(data_type), int(chunk_cols)), "pagan_anc_fit_predict_bytes")


ANC_NNI_CONVERGED, ANC_NNI_MAX_ROUNDS, ANC_NNI_STALLED = 0, 1, 2
ANC_NNI_FIT_ROUNDS = 8           # align_refined(tree_search="nni", branch_lengths="ml"): the fit's rounds after every accepted round
ANC_NNI_STATUS = {ANC_NNI_CONVERGED: "converged", ANC_NNI_MAX_ROUNDS: "max_rounds", ANC_NNI_STALLED: "stalled"}


def _anc_nni_opts(min_gain, max_rounds, fit_rounds, t_min, t_max, tol):
    return CAncNniOpts(float(min_gain), float(t_min), float(t_max), float(tol), int(max_rounds), int(fit_rounds), 0)


def _anc_nni_info(ci):
    info = struct_dict(ci)
    info["status"] = ANC_NNI_STATUS.get(info["status"], info["status"])
    return info


def anc_nni_gains(left, right, branch, rows, data_type=0, base_freq=None):
    """pagan_anc_nni_gains: the log likelihood gains of both nearest-neighbour interchanges around every internal edge, one
    evaluation on the current device.  Returns a dict, row k for internal node n + k: kind (int32 [n - 1]: 0 no candidate, 1
    ordinary, 2 the root edge), M, gain (float64) and E, degenerate (int64) [n - 1, 2] (column 0: a and b exchanged, column 1:
    d and b); loglik (anc_reconstruct's); info."""
    n, le, ri, br = _anc_tree_args(left, right, branch, rows)
    _keep, bfp = _base_freq(base_freq)
    kind = np.zeros(n - 1, np.int32)
    M, gain = np.zeros((n - 1, 2), np.float64), np.zeros((n - 1, 2), np.float64)
    E, deg = np.zeros((n - 1, 2), np.int64), np.zeros((n - 1, 2), np.int64)
    loglik, ci = C.c_double(0.0), CAncNniInfo()
    check(_lib().pagan_anc_nni_gains(n, _ip(le), _ip(ri), _dp(br), _c_strings(rows), int(data_type), bfp, _ip(kind), _dp(M),
                                     E.ctypes.data_as(_i64p), _dp(gain), deg.ctypes.data_as(_i64p), C.byref(loglik), C.byref(ci)),
          "pagan_anc_nni_gains")
    return {"kind": kind, "M": M, "E": E, "gain": gain, "degenerate": deg, "loglik": loglik.value, "info": _anc_nni_info(ci)}


def anc_nni_apply(left, right, branch, node, k):
    """pagan_anc_nni_apply (host only): the swap k (1: a and b, 2: d and b) at the candidate `node`, the internal nodes renumbered in
    post-order.  Returns (left, right, branch, perm) as lists; perm[old id] = new id."""
    le, ri = np.ascontiguousarray(left, np.int32), np.ascontiguousarray(right, np.int32)
    br = np.ascontiguousarray(branch, np.float64)
    n = len(le) + 1
    if len(ri) != n - 1 or len(br) != 2 * n - 1:
        raise ValueError("left, right hold n - 1 entries and branch 2 n - 1")
    lo, ro, bo, perm = np.zeros(n - 1, np.int32), np.zeros(n - 1, np.int32), np.zeros(2 * n - 1, np.float64), np.zeros(2 * n - 1, np.int32)
    check(_lib().pagan_anc_nni_apply(n, _ip(le), _ip(ri), _dp(br), int(node), int(k), _ip(lo), _ip(ro), _dp(bo), _ip(perm)), "pagan_anc_nni_apply")
    return [int(x) for x in lo], [int(x) for x in ro], [float(x) for x in bo], [int(x) for x in perm]


def anc_nni_select(left, right, gain, degenerate, min_gain=1e-3):
    """pagan_anc_nni_select (host only): the swaps a round applies, from gain and degenerate [n - 1, 2] as anc_nni_gains returns
    them: [(node, k)] in the order taken -- descending gain, no two edges sharing a node."""
    le, ri = np.ascontiguousarray(left, np.int32), np.ascontiguousarray(right, np.int32)
    n = len(le) + 1
    g, d = np.ascontiguousarray(gain, np.float64).reshape(-1), np.ascontiguousarray(degenerate, np.int64).reshape(-1)
    if len(ri) != n - 1 or len(g) != 2 * (n - 1) or len(d) != 2 * (n - 1):
        raise ValueError("left, right hold n - 1 entries, gain and degenerate (n - 1) x 2")
    nodes, ks = np.zeros(n - 1, np.int32), np.zeros(n - 1, np.int32)
    count = check(_lib().pagan_anc_nni_select(n, _ip(le), _ip(ri), _dp(g), d.ctypes.data_as(_i64p), float(min_gain), _ip(nodes), _ip(ks)),
                  "pagan_anc_nni_select")
    return [(int(nodes[i]), int(ks[i])) for i in range(count)]


def anc_nni_search(left, right, branch, rows, data_type=0, base_freq=None, min_gain=1e-3, max_rounds=32, fit_rounds=0, t_min=1e-6,
                   t_max=10.0, tol=1e-6):
    """pagan_anc_nni_search: the likelihood tree search by nearest-neighbour interchanges from the given tree, on the current device.
    Returns a dict: left, right, branch (the final tree, lists), loglik (the accepted log likelihoods, the start first: never
    decreasing), swaps (dicts: round, node in that round's ids, k, joint, gain), info (status as "converged" / "max_rounds" /
    "stalled", rounds, swaps, loglik_start, loglik_end, the stages' device ms, ...)."""
    n, le, ri, br = _anc_tree_args(left, right, branch, rows)
    _keep, bfp = _base_freq(base_freq)
    o = _anc_nni_opts(min_gain, max_rounds, fit_rounds, t_min, t_max, tol)
    rounds = int(max(max_rounds, 0))
    lo, ro, bo = np.zeros(n - 1, np.int32), np.zeros(n - 1, np.int32), np.zeros(2 * n - 1, np.float64)
    hist, ci, count = np.zeros(rounds + 1, np.float64), CAncNniInfo(), C.c_int32(0)
    cap = rounds * max(n - 1, 1)
    swaps = (CAncNniSwap * max(cap, 1))()
    k = check(_lib().pagan_anc_nni_search(n, _ip(le), _ip(ri), _dp(br), _c_strings(rows), int(data_type), bfp, C.byref(o), _ip(lo), _ip(ro),
                                          _dp(bo), _dp(hist), len(hist), swaps, cap, C.byref(count), C.byref(ci)), "pagan_anc_nni_search")
    return {"left": [int(x) for x in lo], "right": [int(x) for x in ro], "branch": [float(x) for x in bo], "loglik": hist[:k].copy(),
            "swaps": [struct_dict(swaps[i]) for i in range(min(count.value, cap))], "info": _anc_nni_info(ci)}


def anc_nni_predict_bytes(n_leaves, columns, data_type, chunk_cols=0):
    """pagan_anc_nni_predict_bytes (host only): device bytes anc_nni_search or anc_nni_gains allocates at most."""
    return check(_lib().pagan_anc_nni_predict_bytes(int(n_leaves), int(columns), int(data_type), int(chunk_cols)), "pagan_anc_nni_predict_bytes")


class Ancestral:
    """What Msa.ancestral() leaves: loglik, col_loglik [L], best / best_p [n - 1, L], info, and the overlaid rows."""

    def __init__(self, msa, loglik, col_loglik, best, best_p, info):
        self._msa, self.loglik, self.col_loglik, self.best, self.best_p, self.info = msa, loglik, col_loglik, best, best_p, info

    def row(self, node):
        """pagan_msa_ancestral_row: the node's row with every non-gap character of an ancestor replaced by its most probable state."""
        m = self._msa
        n = m._L.pagan_msa_alignment_length(m._h)
        buf = C.create_string_buffer(n + 1)
        check(m._L.pagan_msa_ancestral_row(m._h, node, buf), "pagan_msa_ancestral_row")
        return buf.raw[:n].decode()

    def support(self, node):
        """pagan_msa_ancestral_support: the posterior of the shown state per column (float32), -1 at gaps."""
        m = self._msa
        buf = np.zeros(int(self.info["columns"]), np.float32)
        check(m._L.pagan_msa_ancestral_support(m._h, node, _fp(buf)), "pagan_msa_ancestral_support")
        return buf

    def write_fasta(self, path, chars_by_line=60):
        """pagan_msa_write_fasta_ancestral: write_fasta(include_internal=True)'s file with the overlaid rows."""
        m = self._msa
        check(m._L.pagan_msa_write_fasta_ancestral(m._h, str(path).encode(), chars_by_line), "pagan_msa_write_fasta_ancestral")


def differing_clades(newick_a, newick_b):
    """The clades (leaf sets under the internal nodes) of tree a that tree b does not have."""
    from . import synth

    def clades(newick):
        out = set()

        def walk(t):
            if t[0] == "leaf":
                return frozenset([t[1]])
            s = walk(t[1]) | walk(t[2])
            out.add(s)
            return s
        walk(synth.parse_newick(newick))
        return out
    return len(clades(newick_a) - clades(newick_b))


def newick_arrays(names, newick):
    """(left, right, branch) of a rooted binary Newick in the walk's ids: leaf k is names[k], the internal nodes n, n + 1, ... in the
    order their brackets close, branch [2 n - 1] the length above every node as written (the root's 0)."""
    from . import synth
    n = len(names)
    index = {name: k for k, name in enumerate(names)}
    left, right, branch = [], [], [0.0] * (2 * n - 1)

    def visit(t):
        if t[0] == "leaf":
            v = index[t[1]]
        else:
            a, b = visit(t[1]), visit(t[2])
            v = n + len(left)
            left.append(a)
            right.append(b)
        branch[v] = float(t[-1])
        return v
    if visit(synth.parse_newick(newick)) != 2 * n - 2:
        raise ValueError("the tree does not hold every name once")
    branch[-1] = 0.0
    return left, right, branch


def arrays_newick(names, left, right, branch):
    """newick_arrays' inverse: the tree as a Newick string, the lengths printed %.17g (the root's is not printed)."""
    n = len(names)
    text = list(names) + [None] * (n - 1)
    for k in range(n - 1):
        text[n + k] = "(%s:%.17g,%s:%.17g)" % (text[left[k]], branch[left[k]], text[right[k]], branch[right[k]])
    return text[2 * n - 2] + ";"


def dna_base_frequencies(seqs):
    """The walk's empirical base frequencies of DNA sequences: the counts of A, C, G, T as floats, each over their float sum."""
    counts = [np.float32(min(sum(s.count(c) for s in seqs), 1 << 24)) for c in "ACGT"]
    total = counts[0] + counts[1] + counts[2] + counts[3]
    return [c / total for c in counts]


def align_refined(names, seqs, rounds=1, newick=None, branch_lengths=None, tree_method="upgma", tree_search=None, **msa_kwargs):
    """Align, read the guide tree off the alignment, align again on it: walks once exactly as Msa(names, seqs, newick,
    **msa_kwargs).align() does, then up to `rounds` times takes T = msa.alignment_tree() and walks again on T, stopping when
    T is the tree just walked (the walk is deterministic: a fixpoint).  Returns the last Msa (the earlier ones are closed) with
    .history: one dict per walk -- newick, alignment_length, score (the sum of the node scores) and changed_clades (the clades
    of its tree the previous walk's tree does not have; 0 for the first).
    branch_lengths="ml": T keeps alignment_tree()'s topology and takes its lengths from anc_fit_branches over the current
    alignment's rows, started from alignment_tree()'s lengths (DNA: under the walk's base frequencies); every history entry
    gains loglik (Msa.ancestral()'s, of the walk's alignment under the lengths it aligned with) and fit (status, rounds,
    loglik_start, loglik_end of the fit that made its tree; None for the first walk).
    tree_method="nj": the first tree (where no newick is given) and every tree read off an alignment are neighbour-joining trees
    (Msa's tree_method, alignment_tree's method); it composes with branch_lengths="ml".
    tree_search="nni": after T is read off the alignment (and fitted, with branch_lengths="ml"), anc_nni_search runs from T over the
    current alignment's rows -- with "ml" with fit_rounds=ANC_NNI_FIT_ROUNDS, so that every accepted tree's lengths are fitted -- and
    the walk goes on the tree it finds; every history entry gains search (status, rounds, swaps, loglik_start, loglik_end of the
    search that made its tree; None for the first walk)."""
    if branch_lengths not in (None, "ml"):
        raise ValueError("branch_lengths is None or 'ml'")
    if tree_search not in (None, "nni"):
        raise ValueError("tree_search is None or 'nni'")
    _tree_method(tree_method)
    ml = branch_lengths == "ml"
    msa = Msa(names, seqs, newick, tree_method=tree_method, **msa_kwargs).align()
    history = []

    def record(m, before, fit=None, search=None):
        history.append({"newick": m.newick, "alignment_length": len(m.alignment()[0]),
                        "score": float(sum(m.node_info(k).score for k in range(m.n_internal))),
                        "changed_clades": 0 if before is None else differing_clades(m.newick, before)})
        if ml:
            history[-1]["loglik"] = m.ancestral().loglik
            history[-1]["fit"] = None if fit is None else {k: fit["info"][k] for k in ("status", "rounds", "loglik_start", "loglik_end")}
        if tree_search:
            history[-1]["search"] = None if search is None else {k: search["info"][k] for k in ("status", "rounds", "swaps", "loglik_start", "loglik_end")}
    record(msa, None)
    for _ in range(int(rounds)):
        tree, fit, search = msa.alignment_tree(method=tree_method), None, None
        if ml or tree_search:
            left, right, branch = newick_arrays(list(names), tree)
            data_type = msa.data_type
            base_freq = dna_base_frequencies(seqs) if data_type == 1 else None
        if ml:
            fit = anc_fit_branches(left, right, branch, msa.alignment(), data_type, base_freq)
            branch = fit["branch"]
            tree = arrays_newick(list(names), left, right, branch)
        if tree_search:
            search = anc_nni_search(left, right, branch, msa.alignment(), data_type, base_freq, fit_rounds=ANC_NNI_FIT_ROUNDS if ml else 0)
            tree = arrays_newick(list(names), search["left"], search["right"], search["branch"])
        if tree == msa.newick:
            break
        before = msa.newick
        msa.close()
        msa = Msa(names, seqs, tree, **msa_kwargs).align()
        record(msa, before, fit, search)
    msa.history = history
    return msa


def _job_copy(j):
    """(Graph, Graph, Model, Band|None) copies of a borrowed CJob."""
    left, right = _graph_from_view(j.left.contents), _graph_from_view(j.right.contents)
    m = j.model.contents
    S = m.n_states
    table = np.ctypeslib.as_array(m.log_score, shape=(S * S,)).copy()
    model = abi.Model(table.reshape(S, S).T, m.log_gap_open, m.log_gap_ext, m.log_gap_end_ext, m.log_non_gap)
    band = None
    if j.band:
        b = j.band.contents
        band = abi.Band(np.ctypeslib.as_array(b.upper, shape=(b.n,)).copy(), np.ctypeslib.as_array(b.lower, shape=(b.n,)).copy())
    return left, right, model, band


class Pileup(Handle):
    """Reads_aligner::pileup_alignment mirror: read 0 is the reference, every further read is aligned (GPU) against the
    growing root and joins it when it overlaps well enough."""
    _destroy = "pagan_pileup_destroy"

    def __init__(self, names, seqs, **opts):
        L = _lib()
        o = CPileupOpts()
        L.pagan_pileup_default_opts(C.byref(o))
        for k, v in opts.items():
            if not hasattr(o, k):
                raise TypeError("unknown option %s" % k)
            setattr(o, k, v)
        self.n = len(names)
        na, sa = _c_strings(names), _c_strings(seqs)
        self._h = C.c_void_p()
        check(L.pagan_pileup_create(self.n, na, sa, C.byref(o), C.byref(self._h)), "pagan_pileup_create")
        self._L = L

    def set_batch_backend(self, fn):
        """TEST SEAM: `fn` stands in for pagan_dp_align_batch (see Msa.set_batch_backend)."""
        self._backend = BATCH_FN(fn) if fn is not None else C.cast(None, BATCH_FN)
        self._L.pagan_pileup_set_batch_backend(self._h, self._backend, None)

    def align(self):
        check(self._L.pagan_pileup_align(self._h), "pagan_pileup_align")
        return self

    @property
    def n_steps(self):
        return self._L.pagan_pileup_n_steps(self._h)

    def step(self, k):
        s = CPileupStep()
        self._L.pagan_pileup_step_info(self._h, k, C.byref(s))
        return s

    def step_job(self, k):
        j = abi.CJob()
        check(self._L.pagan_pileup_step_job(self._h, k, C.byref(j)), "pagan_pileup_step_job")
        return _job_copy(j)

    def step_result(self, k):
        r = abi.CResult()
        check(self._L.pagan_pileup_step_result(self._h, k, C.byref(r)), "pagan_pileup_step_result")
        return abi.Result(r)

    def alignment(self):
        n = self._L.pagan_pileup_alignment_length(self._h)
        buf = C.create_string_buffer(n + 1)
        rows = []
        for k in range(self.n):
            ln = self._L.pagan_pileup_alignment_row(self._h, k, buf)
            rows.append(buf.raw[:ln].decode())
        return rows


class Msa(Handle):
    """Progressive alignment of sequences on a rooted binary guide tree (Node mirror)."""
    _destroy = "pagan_msa_destroy"

    def __init__(self, names, seqs, newick=None, sample_on_device=0, posterior_decode=0, decode_gap_weight=0.5, expected_counts=0,
                 indel_model=None, tree_method="upgma", **opts):
        """newick=None: the guide tree is made from the sequences (guide_tree with the walk's data_type, on the current
        device; tree_method="nj": by neighbour joining); either way the tree walked is kept as self.newick.
        opts: fields of pagan_msa_opts.  sample_on_device=1 (pagan_msa_set_sampler): with sample_path set, the nodes' paths
        are drawn by pg_fb_sample on the device instead of on the host behind a download of the forward matrix.
        posterior_decode=1 (pagan_msa_set_decoder): a node's result is the maximum expected accuracy path of its posteriors,
        gaps weighted by decode_gap_weight.  expected_counts=1 (pagan_msa_set_counts): every node's forward/backward pass also
        leaves its expected transition counts (node_counts, expected_counts).  indel_model=(ins_rate, del_rate, gap_ext,
        end_gap_ext) (pagan_msa_set_indel_model): the walk's indel model; a negative entry keeps the data type's default."""
        _tree_method(tree_method)
        L = _lib()
        o = CMsaOpts()
        L.pagan_msa_default_opts(C.byref(o))
        for k, v in opts.items():
            if not hasattr(o, k):
                raise TypeError("unknown option %s" % k)
            setattr(o, k, v)
        self.n = len(names)
        self.names = list(names)
        self._h = C.c_void_p()
        if newick is None:
            newick = guide_tree(names, seqs, data_type=o.data_type, method=tree_method)
        self.newick = newick
        na, sa = _c_strings(names), _c_strings(seqs)
        check(L.pagan_msa_create(self.n, na, sa, newick.encode(), C.byref(o), C.byref(self._h)), "pagan_msa_create")
        self._L = L
        if sample_on_device:
            check(L.pagan_msa_set_sampler(self._h, int(sample_on_device)), "pagan_msa_set_sampler")
        if posterior_decode:
            check(L.pagan_msa_set_decoder(self._h, int(posterior_decode), float(decode_gap_weight)), "pagan_msa_set_decoder")
        if expected_counts:
            check(L.pagan_msa_set_counts(self._h, int(expected_counts)), "pagan_msa_set_counts")
        if indel_model is not None:
            check(L.pagan_msa_set_indel_model(self._h, *[float(v) for v in indel_model]), "pagan_msa_set_indel_model")

    def align(self):
        check(self._L.pagan_msa_align(self._h), "pagan_msa_align")
        return self

    @property
    def n_internal(self):
        return self._L.pagan_msa_n_internal(self._h)

    @property
    def data_type(self):
        return self._L.pagan_msa_data_type(self._h)

    # ---- the walk one round at a time (one process per GPU; see dist.align_sharded) ----
    def ready(self):
        ids = np.zeros(max(self.n, 1), np.int32)
        cnt = self._L.pagan_msa_ready(self._h, _ip(ids), int(ids.shape[0]))
        return [int(x) for x in ids[:cnt]]

    @property
    def remaining(self):
        return self._L.pagan_msa_remaining(self._h)

    def node_cost(self, node):
        return int(self._L.pagan_msa_node_cost(self._h, node))

    def align_nodes(self, nodes):
        ids = np.ascontiguousarray(nodes, np.int32)
        check(self._L.pagan_msa_align_nodes(self._h, int(ids.shape[0]), _ip(ids)), "pagan_msa_align_nodes")

    def export_result(self, node):
        need = check(self._L.pagan_msa_export_result(self._h, node, None, 0), "pagan_msa_export_result")
        buf = np.zeros(need, np.uint8)
        self._L.pagan_msa_export_result(self._h, node, buf.ctypes.data_as(C.c_void_p), need)
        return buf

    def import_result(self, buf):
        b = np.ascontiguousarray(buf, np.uint8)
        check(self._L.pagan_msa_import_result(self._h, b.ctypes.data_as(C.c_void_p), int(b.shape[0])), "pagan_msa_import_result")

    def node_device(self, k):
        return self._L.pagan_msa_node_device(self._h, k)

    def set_batch_backend(self, fn):
        """TEST SEAM: `fn(n, jobs, opts, out, user) -> rc` stands in for pagan_dp_align_batch (None: the HIP path)."""
        self._backend = BATCH_FN(fn) if fn is not None else C.cast(None, BATCH_FN)
        self._L.pagan_msa_set_batch_backend(self._h, self._backend, None)

    def finish(self, lazy=False):
        """After the last round.  lazy: the parent graphs of imported nodes that nobody needed, and the rows, are built by
        the first call that asks for them (alignment(), write_fasta(), node_graph()) instead of now."""
        check((self._L.pagan_msa_finish_lazy if lazy else self._L.pagan_msa_finish)(self._h), "pagan_msa_finish")
        return self

    @property
    def parents_built(self):
        """parent graphs this process has built so far (rank mode: the nodes it aligned and the imported ones it needed)"""
        return self._L.pagan_msa_parents_built(self._h)

    def node_info(self, k):
        info = CNodeInfo()
        self._L.pagan_msa_node_info(self._h, k, C.byref(info))
        return info

    def node_cjob(self, k):
        """Borrowed CJob (pointers into the Msa; valid while it lives)."""
        j = abi.CJob()
        check(self._L.pagan_msa_node_job(self._h, k, C.byref(j)), "pagan_msa_node_job")
        return j

    def node_job(self, k):
        """(Graph, Graph, Model, Band|None) copies of node k's aligner inputs."""
        return _job_copy(self.node_cjob(k))

    def node_result(self, k):
        r = abi.CResult()
        check(self._L.pagan_msa_node_result(self._h, k, C.byref(r)), "pagan_msa_node_result")
        return abi.Result(r)

    # ---- what the forward/backward pass left at a node (full_probability= / sample_path=) ----
    def node_fb(self, k):
        """(log_fwd, log_bwd, device ms of the sweeps, device ms of support + marginals) of internal node k."""
        out = (C.c_double * 4)()
        check(self._L.pagan_msa_node_fb(self._h, k, out), "pagan_msa_node_fb")
        return tuple(out)

    def node_decode(self, k):
        """(objective, steps, device ms of fill + trace) of internal node k's decoded path (posterior_decode=1)."""
        out = (C.c_double * 3)()
        check(self._L.pagan_msa_node_decode(self._h, k, out), "pagan_msa_node_decode")
        return tuple(out)

    def node_counts(self, k, emissions=None):
        """Node k's expected counts (expected_counts=1): the dict FullProbability.expected_counts returns.  emissions: None
        takes the table where the walk keeps one (DNA)."""
        v = abi.CModelProb()
        check(self._L.pagan_msa_node_model_prob(self._h, k, C.byref(v)), "pagan_msa_node_model_prob")
        S = v.n_states
        if emissions is None:
            emissions = self.data_type == 1
        trans = np.zeros(12, np.float64)
        emit = np.zeros(S * S, np.float64) if emissions else None
        check(self._L.pagan_msa_node_counts(self._h, k, _dp(trans), _dp(emit) if emissions else None), "pagan_msa_node_counts")
        return {"trans": trans[:9].reshape(3, 3).copy(), "end": trans[9:].copy(), "emit": emit.reshape(S, S).T.copy() if emissions else None}

    def expected_counts(self):
        """The sum of the expected counts over the nodes this process aligned: {"trans", "end", "emit", "nodes": [k, ...],
        "dists": [node k's distance, ...], "node_counts": [node k's dict, ...]} -- the last two are what fit_indel takes."""
        out = {"trans": np.zeros((3, 3)), "end": np.zeros(3), "emit": None, "nodes": [], "dists": [], "node_counts": []}
        for k in range(self.n_internal):
            if self.node_device(k) < 0:
                continue
            c = self.node_counts(k)
            out["trans"] += c["trans"]; out["end"] += c["end"]
            if c["emit"] is not None:
                out["emit"] = c["emit"].copy() if out["emit"] is None else out["emit"] + c["emit"]
            out["nodes"].append(k); out["dists"].append(self.node_info(k).dist); out["node_counts"].append(c)
        return out

    def node_support(self, k):
        """Posterior of every column's own cell along node k's path; -1 at skip columns."""
        out = np.zeros(self.node_result(k).cols.shape[0], np.float64)
        check(self._L.pagan_msa_node_support(self._h, k, _dp(out)), "pagan_msa_node_support")
        return out

    def node_marginals(self, k):
        """Node k's site marginals (full_probability=2): the dict FullProbability.site_marginals returns."""
        info = self.node_info(k)
        Lx, Ly = info.left_sites - 1, info.right_sites - 1
        out = {"pX": np.zeros(Lx), "pM_left": np.zeros(Lx), "best_j": np.zeros(Lx, np.int32), "best_p_left": np.zeros(Lx),
               "pY": np.zeros(Ly), "pM_right": np.zeros(Ly), "best_i": np.zeros(Ly, np.int32), "best_p_right": np.zeros(Ly)}
        args = [out[k_].ctypes.data_as(_i32p if k_ in ("best_j", "best_i") else _f64p)
                for k_ in ("pX", "pM_left", "best_j", "best_p_left", "pY", "pM_right", "best_i", "best_p_right")]
        check(self._L.pagan_msa_node_marginals(self._h, k, *args), "pagan_msa_node_marginals")
        return out

    def node_model_prob(self, k):
        """abi.ModelProb copy of the probability-space model node k's forward/backward pass takes."""
        v = abi.CModelProb()
        check(self._L.pagan_msa_node_model_prob(self._h, k, C.byref(v)), "pagan_msa_node_model_prob")
        S = v.n_states
        score = np.ctypeslib.as_array(v.score, shape=(S * S,)).copy()
        return abi.ModelProb(score.reshape(S, S).T, v.gap_open, v.gap_ext, v.non_gap)

    def support_row(self, node):
        """Node `node`'s column support on the final alignment's columns (float32, -1 where the node has no column)."""
        n = check(self._L.pagan_msa_alignment_length(self._h), "pagan_msa_alignment_length")
        buf = np.zeros(n, np.float32)
        check(self._L.pagan_msa_support_row(self._h, node, _fp(buf)), "pagan_msa_support_row")
        return buf

    def node_graph(self, node):
        return HGraph(self._L.pagan_msa_node_graph(self._h, node), owned=False, keep=self)

    def timing(self):
        t = CTiming()
        self._L.pagan_msa_timing_get(self._h, C.byref(t))
        return struct_dict(t)

    def alignment(self):
        n = self._L.pagan_msa_alignment_length(self._h)
        rows = []
        buf = C.create_string_buffer(n + 1)
        for k in range(self.n):
            self._L.pagan_msa_alignment_row(self._h, k, buf)
            rows.append(buf.raw[:n].decode())
        return rows

    def alignment_tree(self, with_info=False, method="upgma"):
        """pagan_msa_alignment_tree: the guide tree made from this walk's own alignment -- aln_tree over the leaf rows under the
        walk's names and data type (with_info: and the info dict).  PaganError(PAGAN_E_ARG) before the rows exist.
        method="nj": aln_tree(method="nj") over the same rows."""
        if _tree_method(method):
            check(self._L.pagan_msa_alignment_length(self._h), "pagan_msa_alignment_tree")
            return aln_tree(self.names, self.alignment(), data_type=self.data_type, with_info=with_info, method="nj")
        ci = CAlnInfo()
        newick = _newick_call(lambda buf, cap: self._L.pagan_msa_alignment_tree(self._h, buf, cap, C.byref(ci)),
                              "pagan_msa_alignment_tree", self.names)
        return (newick, struct_dict(ci)) if with_info else newick

    def ancestral(self):
        """pagan_msa_ancestral: marginal ancestral states of the finished walk on the current device -- its leaf rows, its tree,
        the branch lengths it aligned under.  Returns an Ancestral; PaganError(PAGAN_E_ARG) before the rows exist."""
        n = self._L.pagan_msa_alignment_length(self._h)
        col = np.zeros(max(n, 0), np.float64)
        loglik, ci = C.c_double(0.0), CAncInfo()
        check(self._L.pagan_msa_ancestral(self._h, 0, C.byref(loglik), _dp(col), C.byref(ci)), "pagan_msa_ancestral")
        L = int(ci.columns)
        bp, pp = _u8p(), _f32p()
        check(self._L.pagan_msa_ancestral_best(self._h, C.byref(bp), C.byref(pp)), "pagan_msa_ancestral_best")
        shape = (self.n - 1, L)
        if L:
            best, best_p = np.ctypeslib.as_array(bp, shape=shape).copy(), np.ctypeslib.as_array(pp, shape=shape).copy()
        else:
            best, best_p = np.zeros(shape, np.uint8), np.zeros(shape, np.float32)
        return Ancestral(self, loglik.value, col[:L].copy(), best, best_p, struct_dict(ci))

    def fit_branches(self, t_min=1e-6, t_max=10.0, tol=1e-6, max_rounds=32):
        """pagan_msa_fit_branches: the branch lengths of largest likelihood for the finished walk's alignment on its tree, from the
        lengths it aligned under, on the current device.  Returns a dict: branch [2 n - 1] by node id, newick (the walk's
        topology and names with the fitted lengths), info (anc_fit_branches').  The walk itself is not changed."""
        o, ci = _anc_fit_opts(t_min, t_max, tol, max_rounds), CAncFitInfo()
        out = np.zeros(2 * self.n - 1, np.float64)
        newick = _newick_call(lambda buf, cap: self._L.pagan_msa_fit_branches(self._h, C.byref(o), _dp(out), buf, cap, C.byref(ci)),
                              "pagan_msa_fit_branches", self.names)
        return {"branch": out, "newick": newick, "info": _anc_fit_info(ci)}

    def search_tree(self, min_gain=1e-3, max_rounds=32, fit_rounds=0, t_min=1e-6, t_max=10.0, tol=1e-6):
        """pagan_msa_search_tree: anc_nni_search over the finished walk's alignment, from its tree and the lengths it aligned
        under, on the current device.  Returns a dict: newick (the tree found, under the walk's names), info (anc_nni_search's).
        The walk itself is not changed."""
        o, ci = _anc_nni_opts(min_gain, max_rounds, fit_rounds, t_min, t_max, tol), CAncNniInfo()
        newick = _newick_call(lambda buf, cap: self._L.pagan_msa_search_tree(self._h, C.byref(o), buf, cap, C.byref(ci)),
                              "pagan_msa_search_tree", self.names)
        return {"newick": newick, "info": _anc_nni_info(ci)}

    def alignment_all(self):
        """Rows of every node: leaves 0..n-1, then the internal nodes (ancestors) in alignment order."""
        n = self._L.pagan_msa_alignment_length(self._h)
        rows = []
        buf = C.create_string_buffer(n + 1)
        for k in range(2 * self.n - 1):
            self._L.pagan_msa_alignment_row(self._h, k, buf)
            rows.append(buf.raw[:n].decode())
        return rows

    def write_fasta(self, path, chars_by_line=60, include_internal=False):
        """The rows as FASTA in guide-tree order (Fasta_reader::write_fasta over Node::get_alignment); with
        include_internal the ancestors' rows too, in Node::get_all_nodes order."""
        check(self._L.pagan_msa_write_fasta_nodes(self._h, str(path).encode(), chars_by_line, 1 if include_internal else 0), "pagan_msa_write_fasta")
