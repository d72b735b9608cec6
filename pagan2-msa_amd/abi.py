"""ctypes mirror of include/pagan_dp.h and numpy-backed holders for its structs.

Plumbing only: every compute entry point lives in libpagan_dp.so (HIP).  The classes
here keep the numpy arrays alive for as long as the C structs that point into them.
"""
import ctypes as C

import numpy as np

# ---- constants (include/pagan_dp.h) ----------------------------------------------------
PAGAN_OK = 0
PAGAN_E_ARG, PAGAN_E_GRAPH, PAGAN_E_BAND, PAGAN_E_MODEL = -1, -2, -3, -4
PAGAN_E_NODEVICE, PAGAN_E_NOMEM, PAGAN_E_INTERNAL = -5, -6, -7
PAGAN_DP_REACHED, PAGAN_DP_UNREACHABLE = 0, 1
OPT_NO_TERMINAL_EDGES = 1
OPT_NO_REDUCED_TERMINAL_PEN = 2
SAMPLE_NO_TRACES = 1
DECODE_KEEP_MATRIX = 1
X_MAT, Y_MAT, M_MAT = 0, 1, 2
MATCHED, XGAPPED, YGAPPED, XSKIPPED, YSKIPPED = 2, 3, 4, 5, 6

# ---- the short names the prototype tables (PROTOTYPES, host.PROTOTYPES) are written in ------
cint, i32, i64, u8, u32, u64, f32, f64 = C.c_int, C.c_int32, C.c_int64, C.c_uint8, C.c_uint32, C.c_uint64, C.c_float, C.c_double
vp, cp = C.c_void_p, C.c_char_p                     # vp: a pointer to an opaque handle type as well (pagan_batch * ...)
vpp, cpp = C.POINTER(vp), C.POINTER(cp)
_i32p, _i64p, _u8p, _u32p, _f32p, _f64p = (C.POINTER(t) for t in (i32, i64, u8, u32, f32, f64))
_i32pp, _f64pp = C.POINTER(_i32p), C.POINTER(_f64p)


def _ip(a):
    return a.ctypes.data_as(_i32p)


def _fp(a):
    return a.ctypes.data_as(_f32p)


def _dp(a):
    return a.ctypes.data_as(_f64p)


class CGraph(C.Structure):
    _fields_ = [("n_sites", C.c_int32), ("n_edges", C.c_int32), ("state", _i32p), ("bwd_off", _i32p),
                ("bwd_src", _i32p), ("bwd_logw", _f32p), ("bwd_eid", _i32p)]


class CModel(C.Structure):
    _fields_ = [("n_states", C.c_int32), ("log_score", _f32p), ("log_gap_open", C.c_float),
                ("log_gap_ext", C.c_float), ("log_gap_end_ext", C.c_float), ("log_non_gap", C.c_float)]


class CBand(C.Structure):
    _fields_ = [("n", C.c_int32), ("upper", _i32p), ("lower", _i32p)]


class COpts(C.Structure):
    _fields_ = [("flags", C.c_uint32), ("device", C.c_int32)]


class CCol(C.Structure):
    _fields_ = [("left", C.c_int32), ("right", C.c_int32), ("path_state", C.c_int32)]


class CResult(C.Structure):
    _fields_ = [("status", C.c_int32), ("score", C.c_double), ("end_matrix", C.c_int32),
                ("end_x", C.c_int32), ("end_y", C.c_int32), ("end_x_edge", C.c_int32), ("end_y_edge", C.c_int32),
                ("n_cols", C.c_int32), ("cols", C.POINTER(CCol)),
                ("n_left_used", C.c_int32), ("left_used", _i32p),
                ("n_right_used", C.c_int32), ("right_used", _i32p),
                ("cells", C.c_int64), ("fill_ms", C.c_double), ("trace_ms", C.c_double)]


class CJob(C.Structure):
    _fields_ = [("left", C.POINTER(CGraph)), ("right", C.POINTER(CGraph)), ("model", C.POINTER(CModel)),
                ("band", C.POINTER(CBand))]


class Graph:
    """One child Sequence flattened to CSR (pagan_graph)."""

    def __init__(self, state, bwd_off, bwd_src, bwd_logw, bwd_eid, n_edges=None):
        self.state = np.ascontiguousarray(state, dtype=np.int32)
        self.bwd_off = np.ascontiguousarray(bwd_off, dtype=np.int32)
        self.bwd_src = np.ascontiguousarray(bwd_src, dtype=np.int32)
        self.bwd_logw = np.ascontiguousarray(bwd_logw, dtype=np.float32)
        self.bwd_eid = np.ascontiguousarray(bwd_eid, dtype=np.int32)
        self.n_sites = int(self.state.shape[0])
        if n_edges is None:
            n_edges = int(self.bwd_eid.max()) + 1 if self.bwd_eid.size else 0
        self.n_edges = int(n_edges)
        assert self.bwd_off.shape[0] == self.n_sites + 1
        self.c = CGraph(self.n_sites, self.n_edges, _ip(self.state), _ip(self.bwd_off),
                        _ip(self.bwd_src), _fp(self.bwd_logw), _ip(self.bwd_eid))

    @classmethod
    def chain(cls, states):
        """Plain leaf: start, one site per residue, stop; edge k joins site k-1 -> k
        (edge 0 is the reference's unlinked dummy edge, sequence.cpp:164-165)."""
        states = np.asarray(states, dtype=np.int32)
        n = states.shape[0] + 2
        st = np.full(n, -1, np.int32)
        st[1:-1] = states
        off = np.concatenate([[0], np.arange(0, n, dtype=np.int32)]).astype(np.int32)
        src = np.arange(0, n - 1, dtype=np.int32)
        return cls(st, off, src, np.zeros(n - 1, np.float32), np.arange(1, n, dtype=np.int32), n_edges=n)


class Model:
    def __init__(self, log_score, log_gap_open, log_gap_ext, log_gap_end_ext, log_non_gap):
        t = np.asarray(log_score, dtype=np.float32)
        assert t.ndim == 2 and t.shape[0] == t.shape[1]
        self.n_states = int(t.shape[0])
        # log_score(a,b) = table[a + b*S]  (Db_matrix::g is column-major, db_matrix.h:76-83)
        self.table = np.ascontiguousarray(t.T.reshape(-1))
        self.log_score = t
        self.params = tuple(np.float32(x) for x in (log_gap_open, log_gap_ext, log_gap_end_ext, log_non_gap))
        self.c = CModel(self.n_states, _fp(self.table), *[float(x) for x in self.params])


class CModelProb(C.Structure):
    _fields_ = [("n_states", C.c_int32), ("score", _f32p), ("gap_open", C.c_float), ("gap_ext", C.c_float),
                ("non_gap", C.c_float)]


class ModelProb:
    """pagan_model_prob: the model in probability space (forward/backward pass)."""

    def __init__(self, score, gap_open, gap_ext, non_gap):
        t = np.asarray(score, dtype=np.float32)
        assert t.ndim == 2 and t.shape[0] == t.shape[1]
        self.n_states = int(t.shape[0])
        self.table = np.ascontiguousarray(t.T.reshape(-1))       # score(a,b) = table[a + b*S]
        self.score = t
        self.gap_open, self.gap_ext, self.non_gap = (float(np.float32(x)) for x in (gap_open, gap_ext, non_gap))
        self.c = CModelProb(self.n_states, _fp(self.table), self.gap_open, self.gap_ext, self.non_gap)


class Band:
    def __init__(self, upper, lower):
        self.upper = np.ascontiguousarray(upper, dtype=np.int32)
        self.lower = np.ascontiguousarray(lower, dtype=np.int32)
        assert self.upper.shape == self.lower.shape
        self.c = CBand(int(self.upper.shape[0]), _ip(self.upper), _ip(self.lower))


class Result:
    """Python copy of a pagan_result (the C arrays are freed by the producer's free())."""

    def __init__(self, r):
        self.status = r.status
        self.score = r.score
        self.end = (r.end_matrix, r.end_x, r.end_y, r.end_x_edge, r.end_y_edge)
        n = r.n_cols
        if n > 0:
            buf = np.ctypeslib.as_array(C.cast(r.cols, _i32p), shape=(n, 3)).copy()
        else:
            buf = np.zeros((0, 3), np.int32)
        self.cols = buf
        self.left_used = (np.ctypeslib.as_array(r.left_used, shape=(r.n_left_used,)).copy()
                          if r.n_left_used > 0 else np.zeros(0, np.int32))
        self.right_used = (np.ctypeslib.as_array(r.right_used, shape=(r.n_right_used,)).copy()
                           if r.n_right_used > 0 else np.zeros(0, np.int32))
        self.cells = r.cells
        self.fill_ms = r.fill_ms
        self.trace_ms = r.trace_ms

    def same_alignment(self, other):
        """Bit-exact comparison of everything the parent-graph builder consumes."""
        return (self.status == other.status and
                np.float64(self.score).tobytes() == np.float64(other.score).tobytes() and
                self.end == other.end and np.array_equal(self.cols, other.cols) and
                np.array_equal(self.left_used, other.left_used) and
                np.array_equal(self.right_used, other.right_used))


def struct_dict(s):
    """A struct mirror's fields as a dict (the info and timing structs the library fills)."""
    return {name: getattr(s, name) for name, _ in s._fields_}


# C struct name -> mirror, for every struct include/pagan_dp.h declares with a body (host.STRUCTS: both headers')
STRUCTS = {"pagan_graph": CGraph, "pagan_model": CModel, "pagan_band": CBand, "pagan_opts": COpts, "pagan_col": CCol,
           "pagan_result": CResult, "pagan_job": CJob, "pagan_model_prob": CModelProb}

gp, mp, mpp, bp, op, rp, jp, colp = (C.POINTER(t) for t in (CGraph, CModel, CModelProb, CBand, COpts, CResult, CJob, CCol))

# Every entry point of include/pagan_dp.h in the header's order: name -> (restype, (argtypes...)).  A new entry point is one
# line here; tests/test_abi_cpu.py holds the table against the header's prototypes.
PROTOTYPES = {
    "pagan_dp_align": (cint, (gp, gp, mp, bp, op, rp)),
    "pagan_dp_align_batch": (cint, (i32, jp, op, rp)),
    "pagan_result_free": (None, (rp,)),
    "pagan_dp_predict_bytes": (i64, (i32, i32, bp)),
    "pagan_dp_count_cells": (i64, (i32, i32, bp)),
    "pagan_dp_device_count": (cint, ()),
    "pagan_dp_select_device": (cint, (i32,)),
    "pagan_batch_create": (cint, (i32, jp, op, vpp)),
    "pagan_batch_run": (cint, (vp,)),
    "pagan_batch_sync": (cint, (vp,)),
    "pagan_batch_fetch": (cint, (vp, rp)),
    "pagan_batch_last_ms": (cint, (vp, _f64p)),
    "pagan_batch_last_ms_detail": (cint, (vp, _f64p)),
    "pagan_batch_cells": (i64, (vp,)),
    "pagan_batch_destroy": (None, (vp,)),
    "pagan_batch_debug_trace": (cint, (vp, i32, vp, i64)),
    "pagan_batch_debug_segments": (cint, (vp, i32, _i32p, _i32p, i64)),
    "pagan_dp_debug_plan": (cint, (gp, gp, bp, _u8p, i32, _i32p, i32, _i32p, _i32p)),
    "pagan_dp_debug_far": (cint, (gp, gp, bp, _u8p, _u8p, _u8p, _u8p)),
    "pagan_dp_debug_descriptors": (cint, (gp, gp, bp, i32, _i32p, i64)),
    "pagan_dp_debug_strips": (cint, (gp, gp, bp, i32, _i32p, i32, _i64p, _i64p, i64)),
    "pagan_dp_debug_tiles": (cint, (gp, gp, bp, _i32p, i32, _i32p)),
    "pagan_dp_debug_tiles_staircase": (cint, (_i32p, i32)),
    "pagan_dp_debug_compact": (cint, (gp, gp, bp, _i32p, _i32p, _i32p, _i32p, _i32p, _i32p, _i32p)),
    "pagan_dp_debug_route": (cint, (gp, gp, mp, bp, _i32p)),
    "pagan_batch_debug_scores": (cint, (vp, i32, _f64p, i64)),
    "pagan_batch_debug_backptrs": (cint, (vp, i32, _u32p, i64)),
    "pagan_batch_debug_poison": (cint, (vp,)),
    "pagan_batch_debug_followed": (cint, (vp, i32, _i32p)),
    "pagan_batch_debug_poke_bp": (cint, (vp, i32, i32, i32, i32, u32)),
    "pagan_batch_debug_reruns": (cint, (vp,)),
    "pagan_dp_release_cache": (None, ()),
    "pagan_dp_cached_device_bytes": (i64, (i32,)),
    "pagan_fb_run": (cint, (gp, gp, mpp, bp, op, vpp)),
    "pagan_fb_run_batch": (cint, (i32, C.POINTER(gp), C.POINTER(gp), C.POINTER(mpp), C.POINTER(bp), op, vpp)),
    "pagan_fb_totals": (cint, (vp, _f64p, _f64p, _i64p)),
    "pagan_fb_kernel_ms": (cint, (vp, _f64p)),
    "pagan_fb_groups": (cint, (vp,)),
    "pagan_fb_schedule": (cint, (vp,)),
    "pagan_fb_debug_route": (cint, (gp, gp, bp, _i32p)),
    "pagan_fb_debug_plan": (cint, (gp, gp, bp, i32, i32, i32, _i32p, _i64p, i32, _i32p, _i32p, i32, _i32p, i32)),
    "pagan_fb_dump": (cint, (vp, i32, _f64p)),
    "pagan_fb_posterior_cells": (cint, (vp, i32, _i32p, _f64p)),
    "pagan_fb_sample_path": (cint, (vp, _f64p, i32, rp, _i32p, _i32p)),
    "pagan_fb_destroy": (None, (vp,)),
    "pagan_path_cells": (cint, (colp, i32, _i32p)),
    "pagan_fb_path_support": (cint, (vp, colp, i32, _f64p)),
    "pagan_fb_site_marginals": (cint, (vp, _f64p, _f64p, _i32p, _f64p, _f64p, _f64p, _i32p, _f64p)),
    "pagan_fb_site_marginals_batch": (cint, (i32, vpp, _f64pp, _f64pp, _i32pp, _f64pp, _f64pp, _f64pp, _i32pp, _f64pp)),
    "pagan_fb_post_ms": (cint, (vp, _f64p)),
    "pagan_fb_expected_counts": (cint, (vp, _f64p, _f64p)),
    "pagan_fb_expected_counts_batch": (cint, (i32, vpp, _f64pp, _f64pp)),
    "pagan_fb_counts_ms": (cint, (vp, _f64p)),
    "pagan_fb_counts_predict_bytes": (i64, (i32, i32, i32)),
    "pagan_fb_predict_bytes": (i64, (i32, i32, bp)),
    "pagan_fb_predict_bytes_states": (i64, (i32, i32, bp, i32)),
    "pagan_fb_device_bytes": (cint, (vp, C.POINTER(C.c_int64))),
    "pagan_sample_uniforms": (cint, (u64, i32, i32, _f64p)),
    "pagan_sample_uniforms_path": (cint, (u64, i32, i32, i32, _f64p)),
    "pagan_fb_sample_paths_batch": (cint, (i32, vpp, u64, _i32p, i32, u32, vpp)),
    "pagan_fb_sample_paths": (cint, (vp, u64, i32, i32, u32, vpp)),
    "pagan_fb_samples_summary": (cint, (vp, _i32p, _i32p, _i32p, _i32p, _i32p, _f64p)),
    "pagan_fb_samples_visited": (cint, (vp, i32, _i32p, _i32p)),
    "pagan_fb_samples_visited_all": (cint, (vp, _i32p, _i32p)),
    "pagan_fb_samples_result": (cint, (vp, i32, rp)),
    "pagan_fb_samples_ms": (cint, (vp, _f64p)),
    "pagan_fb_sample_predict_bytes": (i64, (i32, i32, i32, u32)),
    "pagan_fb_samples_destroy": (None, (vp,)),
    "pagan_fb_decode_batch": (cint, (i32, vpp, f64, u32, vpp)),
    "pagan_fb_decode": (cint, (vp, f64, u32, vpp)),
    "pagan_fb_decoded_summary": (cint, (vp, _i32p, _f64p, _i32p, _i32p, _i32p)),
    "pagan_fb_decoded_visited": (cint, (vp, _i32p, _i32p)),
    "pagan_fb_decoded_result": (cint, (vp, rp)),
    "pagan_fb_decoded_dump": (cint, (vp, _f64p)),
    "pagan_fb_decoded_ms": (cint, (vp, _f64p)),
    "pagan_fb_decoded_launch": (cint, (vp, _i32p, _i32p)),
    "pagan_fb_debug_decode_route": (cint, (gp, gp, bp)),
    "pagan_fb_decode_predict_bytes": (i64, (i32, i32, bp)),
    "pagan_fb_decoded_destroy": (None, (vp,)),
    "pagan_dp_version": (cp, ()),
}
EXPORTED = list(PROTOTYPES)


def declare(lib, table=PROTOTYPES):
    """Attach the argtypes/restype of every entry point of `table` to the loaded library."""
    for name, (restype, argtypes) in table.items():
        fn = getattr(lib, name)
        fn.argtypes, fn.restype = list(argtypes), restype
    return lib
