"""pagan2-msa_amd: MI355X-native pairwise graph-vs-graph Viterbi aligner (PAGAN2's
Viterbi_alignment hot path) behind the C ABI of include/pagan_dp.h.

Python here is plumbing: it loads libpagan_dp.so (HIP kernels + C ABI, built in-tree by
build.py) and mirrors the reference's call surface for this path:

    align(left, right, model, band=None, flags=0)      <- Viterbi_alignment::align
    align_batch(jobs, flags=0)                          (ready nodes of one tree level)
    Batch(jobs).run() / .fetch()                        (inputs resident in HBM)

There is no CPU fallback: if the library or a HIP device is missing the calls raise.
"""
import ctypes as C
import os

import numpy as np

from . import abi
from .abi import Band, Graph, Model, ModelProb, Result  # noqa: F401
from .abi import _dp, _f64p, _i32p, _i64p, _ip, _u8p, _u32p

_HERE = os.path.dirname(os.path.abspath(__file__))
# PAGAN_DP_LIB: a diagnostic build (tools/build_stamps.sh writes libpagan_dp_stats.so) instead of the product library
LIB_PATH = os.environ.get("PAGAN_DP_LIB") or os.path.join(_HERE, "libpagan_dp.so")
_lib = None


class PaganError(RuntimeError):
    def __init__(self, code, what):
        super().__init__("%s failed with code %d" % (what, code))
        self.code = code


def check(rc, what):
    """The one error path of the C ABI: a negative return value is a PAGAN_E_* code and raises; anything else (PAGAN_OK, a
    count, a size) is handed back."""
    if rc < 0:
        raise PaganError(int(rc), what)
    return rc


def declare(L):
    """Attach argtypes / restype of every entry point of both headers (abi.PROTOTYPES, host.PROTOTYPES) to the library L."""
    from . import host           # (host imports PaganError, check and lib from here at its top: not before they exist)
    return abi.declare(abi.declare(L), host.PROTOTYPES)


def lib():
    """The loaded C-ABI library, every entry point declared.  Raises if it has not been built (see build.py)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError("libpagan_dp.so is missing: run `python -c 'import __graft_entry__ as g; g.build()'`")
        _lib = declare(C.CDLL(LIB_PATH))
    return _lib


def device_count():
    return lib().pagan_dp_device_count()


class Handle:
    """Owner of one handle of the library: _h, the entry point that destroys it (_destroy), close() and __del__.  A handle
    that is borrowed (owned = False) is left alone."""
    _destroy = None
    owned = True

    def close(self):
        if self.owned and self._h:
            getattr(lib(), self._destroy)(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _band(band):
    """The band argument of an entry point: NULL for a full matrix."""
    return C.byref(band.c) if band is not None else None


def _jobs_array(jobs):
    arr = (abi.CJob * len(jobs))()
    for k, (left, right, model, band) in enumerate(jobs):
        arr[k].left = C.pointer(left.c)
        arr[k].right = C.pointer(right.c)
        arr[k].model = C.pointer(model.c)
        arr[k].band = C.pointer(band.c) if band is not None else None
    return arr


def align_batch(jobs, flags=0, device=-1):
    """jobs: list of (Graph left, Graph right, Model, Band|None).  Returns [Result]."""
    L = lib()
    arr = _jobs_array(jobs)
    opts = abi.COpts(flags, device)
    res = (abi.CResult * len(jobs))()
    rc = L.pagan_dp_align_batch(len(jobs), arr, C.byref(opts), res)
    try:
        check(rc, "pagan_dp_align_batch")
        return [Result(r) for r in res]
    finally:
        for r in res:
            L.pagan_result_free(C.byref(r))


def align(left, right, model, band=None, flags=0, device=-1):
    """Mirror of Viterbi_alignment::align (+ define_tunnel's band as an argument)."""
    L = lib()
    opts = abi.COpts(flags, device)
    res = abi.CResult()
    rc = L.pagan_dp_align(C.byref(left.c), C.byref(right.c), C.byref(model.c),
                          _band(band), C.byref(opts), C.byref(res))
    try:
        check(rc, "pagan_dp_align")
        return Result(res)
    finally:
        L.pagan_result_free(C.byref(res))


class FullProbability(Handle):
    """Forward/backward matrices of one alignment on the GPU (the reference's compute_full_score pass:
    --full-probability, posteriors, --sample-path), in log space.

        fb = FullProbability(left, right, model_prob, band)
        fb.log_fwd, fb.log_bwd          log max_end.fwd_score, log match[0][0].bwd_score
        fb.posterior()                  [Lx, Ly, 3] (X, Y, M), compute_posterior_score
        fb.sample_path(u)               Result with the shape of a Viterbi result
        fb.sample_paths(seed, node, K)  K paths drawn on the device (SampledPaths)
        fb.decode(gap_weight)           the maximum expected accuracy path (DecodedPath)
        fb.expected_counts()            expected transition, end and emission counts (pg_fb_counts)
    """

    _destroy = "pagan_fb_destroy"

    def __init__(self, left, right, model_prob, band=None, device=-1, _handle=None):
        self._L = lib()
        self.left, self.right, self.model, self.band = left, right, model_prob, band     # keep the arrays alive
        if _handle is not None:                          # (full_probability_batch: the pair ran in a batch's launches)
            self._h = _handle
        else:
            opts = abi.COpts(0, device)
            self._h = C.c_void_p()
            check(self._L.pagan_fb_run(C.byref(left.c), C.byref(right.c), C.byref(model_prob.c),
                                       _band(band), C.byref(opts), C.byref(self._h)),
                  "pagan_fb_run")
        a, b, c = C.c_double(), C.c_double(), C.c_int64()
        check(self._L.pagan_fb_totals(self._h, C.byref(a), C.byref(b), C.byref(c)), "pagan_fb_totals")
        self.log_fwd, self.log_bwd, self.cells = a.value, b.value, c.value
        kms = (C.c_double * 2)()
        check(self._L.pagan_fb_kernel_ms(self._h, kms), "pagan_fb_kernel_ms")
        self.forward_ms, self.backward_ms = kms[0], kms[1]
        self.groups = self._L.pagan_fb_groups(self._h)       # 1: one-workgroup sweeps; > 1: 64 x 64 blocks, a wave each; 0: LDS-ring sweeps
        self.schedule = self._L.pagan_fb_schedule(self._h)   # 0 one-workgroup kernels, 1 blocks, 2 LDS ring (plain sequences), 3 deep ring (graph pairs in a tunnel)
        self.shape = (left.n_sites - 1, right.n_sites - 1, 3)

    @property
    def device_bytes(self):
        """pagan_fb_device_bytes: what the pass asked of the device pool for its arena."""
        n = C.c_int64()
        check(self._L.pagan_fb_device_bytes(self._h, C.byref(n)), "pagan_fb_device_bytes")
        return n.value

    def _dump(self, which):
        out = np.zeros(self.shape, np.float64)
        check(self._L.pagan_fb_dump(self._h, which, _dp(out)), "pagan_fb_dump")
        return out

    def log_forward(self):
        return self._dump(0)

    def log_backward(self):
        return self._dump(1)

    def posterior(self):
        return self._dump(2)

    def posterior_cells(self, cells):
        c = np.ascontiguousarray(cells, np.int32).reshape(-1, 3)
        out = np.zeros(c.shape[0], np.float64)
        check(self._L.pagan_fb_posterior_cells(self._h, c.shape[0], _ip(c), _dp(out)), "pagan_fb_posterior_cells")
        return out

    def path_support(self, cols):
        """pagan_fb_path_support: the posterior of every column's own cell along a path (Result.cols), -1 at skip columns."""
        c = np.ascontiguousarray(cols, np.int32).reshape(-1, 3)
        out = np.zeros(c.shape[0], np.float64)
        check(self._L.pagan_fb_path_support(self._h, c.ctypes.data_as(abi.colp), c.shape[0], _dp(out)), "pagan_fb_path_support")
        return out

    def site_marginals(self, rows=True, columns=True):
        """pagan_fb_site_marginals: dict of pX, pM_left, best_j, best_p_left ([Lx], rows=True) and pY, pM_right, best_i,
        best_p_right ([Ly], columns=True), reduced on the device."""
        return site_marginals_batch([self], rows, columns)[0]

    def post_ms(self):
        """Device ms of the handle's last gather, row pass, column pass."""
        ms = (C.c_double * 3)()
        check(self._L.pagan_fb_post_ms(self._h, ms), "pagan_fb_post_ms")
        return ms[0], ms[1], ms[2]

    def sample_path(self, u):
        """(Result, visited cells end -> start as rows (i, j, state))."""
        uu = np.ascontiguousarray(u, np.float64)
        res = abi.CResult()
        vis = np.zeros((self.shape[0] + self.shape[1] + 2, 3), np.int32)
        n = C.c_int32()
        rc = self._L.pagan_fb_sample_path(self._h, _dp(uu), int(uu.shape[0]), C.byref(res), _ip(vis), C.byref(n))
        try:
            check(rc, "pagan_fb_sample_path")
            return Result(res), vis[:n.value].copy()
        finally:
            self._L.pagan_result_free(C.byref(res))

    def sample_paths(self, seed, node, n_paths, traces=True):
        """pagan_fb_sample_paths: n_paths paths drawn on the device (pg_fb_sample); path p is what sample_path gives for
        sample_uniforms_path(seed, node, p, Lx + Ly + 1).  Returns a SampledPaths."""
        return sample_paths_batch([self], seed, [node], n_paths, traces)[0]

    def decode(self, gap_weight=0.5, keep_matrix=False):
        """pagan_fb_decode: the maximum expected accuracy path of the pair's posteriors (cell weight: the posterior, times
        gap_weight in a gap state), found on the device.  Returns a DecodedPath."""
        return decode_batch([self], gap_weight, keep_matrix)[0]

    def expected_counts(self, emissions=True):
        """pagan_fb_expected_counts: {"trans": [3, 3] (from, to over X, Y, M), "end": [3] (X-close, Y-close, M-end),
        "emit": [S, S] (left state, right state) or None}, summed on the device.  emissions=True needs n_states <= 32."""
        return expected_counts_batch([self], emissions)[0]

    def counts_ms(self):
        """Device ms of the handle's last counts pass, booked at the batch's first pair."""
        ms = C.c_double()
        check(self._L.pagan_fb_counts_ms(self._h, C.byref(ms)), "pagan_fb_counts_ms")
        return ms.value


class SampledPaths(Handle):
    """pagan_fb_samples: the paths one pg_fb_sample launch drew for a pair -- summaries on the host, traces on the device until
    a path is asked for.  Keeps its FullProbability (and with it the graphs result() reads) alive."""

    _destroy = "pagan_fb_samples_destroy"

    def __init__(self, fb, handle, n_paths, traces):
        self._L = lib()
        self._fb = fb
        self._h = handle
        self.n_paths = int(n_paths)
        self.traces = bool(traces)
        self.max_steps = fb.shape[0] + fb.shape[1]
        ms = C.c_double()
        check(self._L.pagan_fb_samples_ms(self._h, C.byref(ms)), "pagan_fb_samples_ms")
        self.ms = ms.value               # device ms of pg_fb_sample, booked at the batch's first pair

    def summary(self):
        """dict of status, n_steps, n_m, n_x, n_y (int32 [n_paths]) and log_q (float64 [n_paths])."""
        out = {k: np.zeros(self.n_paths, np.int32) for k in ("status", "n_steps", "n_m", "n_x", "n_y")}
        out["log_q"] = np.zeros(self.n_paths, np.float64)
        check(self._L.pagan_fb_samples_summary(self._h, *[_ip(out[k]) for k in ("status", "n_steps", "n_m", "n_x", "n_y")],
                                               _dp(out["log_q"])), "pagan_fb_samples_summary")
        return out

    def visited(self, p):
        """Path p's cells end -> start as rows (i, j, state): FullProbability.sample_path's second value."""
        vis = np.zeros((self.max_steps + 1, 3), np.int32)
        n = C.c_int32()
        check(self._L.pagan_fb_samples_visited(self._h, int(p), _ip(vis), C.byref(n)), "pagan_fb_samples_visited")
        return vis[:n.value].copy()

    def visited_all(self):
        """Every path's cells in one copy of the trace buffer: ([n_paths, Lx + Ly, 3] int32, [n_paths] step counts)."""
        vis = np.zeros((self.n_paths, self.max_steps, 3), np.int32)
        n = np.zeros(self.n_paths, np.int32)
        check(self._L.pagan_fb_samples_visited_all(self._h, _ip(vis), _ip(n)), "pagan_fb_samples_visited_all")
        return vis, n

    def result(self, p):
        """The replay of path p's trace: a Result of FullProbability.sample_path's shape."""
        res = abi.CResult()
        rc = self._L.pagan_fb_samples_result(self._h, int(p), C.byref(res))
        try:
            check(rc, "pagan_fb_samples_result")
            return Result(res)
        finally:
            self._L.pagan_result_free(C.byref(res))


class DecodedPath(Handle):
    """pagan_fb_decoded: the maximum expected accuracy path of one pair -- the summary on the host, the trace (and, with
    keep_matrix, the score matrix) on the device.  Keeps its FullProbability (and with it the graphs result() reads) alive."""

    _destroy = "pagan_fb_decoded_destroy"

    def __init__(self, fb, handle, keep_matrix):
        self._L = lib()
        self._fb = fb
        self._h = handle
        self.keep_matrix = bool(keep_matrix)
        self.shape = fb.shape
        self.max_steps = fb.shape[0] + fb.shape[1]

    def summary(self):
        """dict of status, objective, n_steps, n_m, n_x, n_y and schedule (0 pg_fb_decode_fill, 1 pg_fb_ring_decode)."""
        status, steps, schedule, obj = C.c_int32(), C.c_int32(), C.c_int32(), C.c_double()
        counts = (C.c_int32 * 3)()
        check(self._L.pagan_fb_decoded_summary(self._h, C.byref(status), C.byref(obj), C.byref(steps), counts, C.byref(schedule)),
              "pagan_fb_decoded_summary")
        return {"status": status.value, "objective": obj.value, "n_steps": steps.value, "n_m": counts[0], "n_x": counts[1],
                "n_y": counts[2], "schedule": schedule.value}

    def visited(self):
        """The path's cells end -> start as rows (i, j, state): FullProbability.sample_path's second value."""
        vis = np.zeros((self.max_steps + 1, 3), np.int32)
        n = C.c_int32()
        check(self._L.pagan_fb_decoded_visited(self._h, _ip(vis), C.byref(n)), "pagan_fb_decoded_visited")
        return vis[:n.value].copy()

    def result(self):
        """The replay of the trace: a Result of FullProbability.sample_path's shape (score = log full probability)."""
        res = abi.CResult()
        rc = self._L.pagan_fb_decoded_result(self._h, C.byref(res))
        try:
            check(rc, "pagan_fb_decoded_result")
            return Result(res)
        finally:
            self._L.pagan_result_free(C.byref(res))

    def matrix(self):
        """The score matrix [Lx, Ly, 3] (X, Y, M), -inf outside the band; needs keep_matrix."""
        out = np.zeros(self.shape, np.float64)
        check(self._L.pagan_fb_decoded_dump(self._h, _dp(out)), "pagan_fb_decoded_dump")
        return out

    def launch(self):
        """pagan_fb_decoded_launch: (threads of the fill's workgroup, the ring instance looked the score table up)."""
        t, tab = C.c_int32(), C.c_int32()
        check(self._L.pagan_fb_decoded_launch(self._h, C.byref(t), C.byref(tab)), "pagan_fb_decoded_launch")
        return t.value, bool(tab.value)

    def ms(self):
        """Device ms of the fill and of the trace, booked at the batch's first pair."""
        ms = (C.c_double * 2)()
        check(self._L.pagan_fb_decoded_ms(self._h, ms), "pagan_fb_decoded_ms")
        return ms[0], ms[1]


def decode_batch(fbs, gap_weight=0.5, keep_matrix=False):
    """pagan_fb_decode_batch: the maximum expected accuracy paths of FullProbability handles of one device (the fills side by
    side, one launch of the walks back) -> [DecodedPath, ...]."""
    L = lib()
    n = len(fbs)
    handles = (C.c_void_p * n)(*[fb._h for fb in fbs])
    outs = (C.c_void_p * n)()
    check(L.pagan_fb_decode_batch(n, handles, float(gap_weight), abi.DECODE_KEEP_MATRIX if keep_matrix else 0, outs), "pagan_fb_decode_batch")
    return [DecodedPath(fb, C.c_void_p(outs[k]), keep_matrix) for k, fb in enumerate(fbs)]


def fb_decode_route(left, right, band=None):
    """pagan_fb_debug_decode_route (host only): 1 when the pair's decode would fill on the LDS ring, 0 on pg_fb_decode_fill."""
    return check(lib().pagan_fb_debug_decode_route(C.byref(left.c), C.byref(right.c), _band(band)), "pagan_fb_debug_decode_route")


def fb_decode_predict_bytes(left_sites, right_sites, band=None):
    return lib().pagan_fb_decode_predict_bytes(left_sites, right_sites, _band(band))


def sample_paths_batch(fbs, seed, nodes, n_paths, traces=True):
    """pagan_fb_sample_paths_batch: n_paths paths for each FullProbability of one device in one launch (node k's key is
    (seed, nodes[k])) -> [SampledPaths, ...]."""
    L = lib()
    n = len(fbs)
    ids = np.ascontiguousarray(nodes, np.int32)
    assert ids.shape == (n,)
    handles = (C.c_void_p * n)(*[fb._h for fb in fbs])
    outs = (C.c_void_p * n)()
    check(L.pagan_fb_sample_paths_batch(n, handles, int(seed) & 0xFFFFFFFFFFFFFFFF, _ip(ids), int(n_paths),
                                        0 if traces else abi.SAMPLE_NO_TRACES, outs), "pagan_fb_sample_paths_batch")
    return [SampledPaths(fb, C.c_void_p(outs[k]), n_paths, traces) for k, fb in enumerate(fbs)]


def fb_sample_predict_bytes(left_sites, right_sites, n_paths, traces=True):
    return lib().pagan_fb_sample_predict_bytes(left_sites, right_sites, n_paths, 0 if traces else abi.SAMPLE_NO_TRACES)


def debug_tiles(left, right, band=None):
    """Diagnostic (host only): (tile side, [(tile row, tile column), ...]) the wide-matrix fill kernel would be
    launched over for this job; an empty list when the job cannot be tiled."""
    L = lib()
    cap = ((left.n_sites + 62) // 64 + 1) * ((right.n_sites + 62) // 64 + 1)
    out = np.zeros(2 * cap, np.int32)
    side = C.c_int32()
    n = check(L.pagan_dp_debug_tiles(C.byref(left.c), C.byref(right.c), _band(band), _ip(out), cap, C.byref(side)), "pagan_dp_debug_tiles")
    return side.value, [tuple(int(v) for v in out[2 * k: 2 * k + 2]) for k in range(min(n, cap))]


def debug_tiles_staircase(tiles):
    """Diagnostic (host only): whether a list of (tile row, tile column) pairs is a staircase (include/pagan_dp.h)."""
    a = np.ascontiguousarray(np.array(tiles, np.int32).reshape(-1, 2))
    return bool(check(lib().pagan_dp_debug_tiles_staircase(_ip(a), len(a)), "pagan_dp_debug_tiles_staircase"))


def debug_compact(left, right, band=None):
    """Diagnostic (host only): the compacted numbering the library aligns graphs with many dead sites in:
    dict with keep_left / keep_right (compacted site -> caller's site), slot_left / slot_right (per kept bwd edge: its position
    in the caller's list of its site), upper / lower (the band over the compacted matrices)."""
    L = lib()
    kl = np.zeros(left.n_sites, np.int32); kr = np.zeros(right.n_sites, np.int32)
    sl = np.zeros(max(int(left.bwd_off[-1]), 1), np.int32); sr = np.zeros(max(int(right.bwd_off[-1]), 1), np.int32)
    up = np.zeros(left.n_sites, np.int32); lo = np.zeros(left.n_sites, np.int32)
    n = np.zeros(4, np.int32)
    check(L.pagan_dp_debug_compact(C.byref(left.c), C.byref(right.c), _band(band), _ip(kl), _ip(kr), _ip(sl), _ip(sr), _ip(up), _ip(lo),
                                   _ip(n)), "pagan_dp_debug_compact")
    return {"keep_left": kl[:n[0]].copy(), "keep_right": kr[:n[1]].copy(), "slot_left": sl[:n[2]].copy(), "slot_right": sr[:n[3]].copy(),
            "upper": up[:n[0] - 1].copy(), "lower": lo[:n[0] - 1].copy()}


ROUTES = ("pg_fill_pipe", "pg_fill_pipe (large table)", "pg_fill_tiles_flow", "pg_fill_wavefront", "pg_fill_pipe (row strips)")


def debug_route(left, right, model, band=None):
    """Diagnostic (host only): (fill kernel pagan_batch_create would give this job, dead sites taken out first?, cells of
    the widest anti-diagonal)."""
    n = np.zeros(2, np.int32)
    rc = check(lib().pagan_dp_debug_route(C.byref(left.c), C.byref(right.c), C.byref(model.c), _band(band), _ip(n)), "pagan_dp_debug_route")
    return ROUTES[rc], bool(n[0]), int(n[1])


def debug_strips(left, right, band=None, max_sites=0):
    """Diagnostic (host only): the row strips a wide job would be filled as -- [(first row, last row, first diagonal, last
    diagonal + 1, feeder wave, first column staged, desc)] with desc[d - first diagonal] = (first row on d, last row, cell index
    of the first row's score in the job's arrays, class); [] when max_sites refuses the job."""
    Lx, Ly = left.n_sites - 1, right.n_sites - 1
    cap = Lx // 192 + 2
    desc_cap = (cap + 1) * (Ly + 192 + 64) + 64
    strips = np.zeros(6 * cap, np.int32)
    off = np.zeros(cap + 1, np.int64)
    desc = np.zeros(4 * desc_cap, np.int64)
    n = check(lib().pagan_dp_debug_strips(C.byref(left.c), C.byref(right.c), _band(band), max_sites, _ip(strips), cap,
                                          off.ctypes.data_as(_i64p), desc.ctypes.data_as(_i64p), desc_cap), "pagan_dp_debug_strips")
    desc = desc.reshape(-1, 4)
    return [tuple(int(v) for v in strips[6 * k: 6 * k + 6]) + (desc[off[k]: off[k + 1]].copy(),) for k in range(n)]


FB_ROUTE_INFO = ("diagonals", "widest", "segments", "min_D", "reach_left", "reach_right", "far_cells", "far_diagonals")


def fb_route(left, right, band=None):
    """pagan_fb_debug_route (host only): (schedule code FullProbability would take under the current environment, info dict)."""
    info = np.zeros(8, np.int32)
    rc = check(lib().pagan_fb_debug_route(C.byref(left.c), C.byref(right.c), _band(band), _ip(info)), "pagan_fb_debug_route")
    return rc, dict(zip(FB_ROUTE_INFO, (int(v) for v in info)))


FB_PLAN_HEAD = ("schedule", "groups", "groups_fwd", "groups_bwd", "block", "nsplit", "n_init", "init_dmin", "segments", "n_dfar",
                "decode_route", "decode_block", "table_in_lds")


def fb_plan(left, right, band=None, n_states=4, groups_cap=64, groups_cap_b=64):
    """pagan_fb_debug_plan (host only): everything FullProbability's plan fixes for the pair under the current environment -- a
    dict of the head words (FB_PLAN_HEAD) and the arrays init_at, seg_start, seg_B, dfar."""
    L = lib()
    args = (C.byref(left.c), C.byref(right.c), _band(band), n_states, groups_cap, groups_cap_b)
    head = np.zeros(16, np.int32)
    check(L.pagan_fb_debug_plan(*args, _ip(head), None, 0, None, None, 0, None, 0), "pagan_fb_debug_plan")
    out = dict(zip(FB_PLAN_HEAD, (int(v) for v in head)))
    n_init, nseg, n_dfar = out["n_init"], out["segments"], out["n_dfar"]
    init_at = np.zeros(n_init, np.int64); seg_start = np.zeros(nseg + 1, np.int32); seg_B = np.zeros(nseg, np.int32); dfar = np.zeros(n_dfar, np.int32)
    check(L.pagan_fb_debug_plan(*args, _ip(head), init_at.ctypes.data_as(_i64p), n_init, _ip(seg_start), _ip(seg_B), nseg, _ip(dfar), n_dfar),
          "pagan_fb_debug_plan")
    out.update(init_at=init_at, seg_start=seg_start[:nseg + 1 if nseg else 0], seg_B=seg_B, dfar=dfar)
    return out


def full_probability_batch(pairs, device=-1):
    """pagan_fb_run_batch: [(left, right, model_prob, band or None), ...] -> [FullProbability, ...]; the wide pairs' forward sweeps
    run in one launch and their backward sweeps in another (all pairs side by side on the device)."""
    L = lib()
    n = len(pairs)
    gp, mpp, bp = abi.gp, abi.mpp, abi.bp
    lefts = (gp * n)(*[C.pointer(p[0].c) for p in pairs])
    rights = (gp * n)(*[C.pointer(p[1].c) for p in pairs])
    models = (mpp * n)(*[C.pointer(p[2].c) for p in pairs])
    bands = (bp * n)(*[(C.pointer(p[3].c) if p[3] is not None else bp()) for p in pairs])
    outs = (C.c_void_p * n)()
    opts = abi.COpts(0, device)
    check(L.pagan_fb_run_batch(n, lefts, rights, models, bands, C.byref(opts), outs), "pagan_fb_run_batch")
    return [FullProbability(p[0], p[1], p[2], p[3], device=device, _handle=C.c_void_p(outs[k])) for k, p in enumerate(pairs)]


_MARGINALS = (("pX", 0, "f"), ("pM_left", 0, "f"), ("best_j", 0, "i"), ("best_p_left", 0, "f"),
              ("pY", 1, "f"), ("pM_right", 1, "f"), ("best_i", 1, "i"), ("best_p_right", 1, "f"))


def site_marginals_batch(fbs, rows=True, columns=True):
    """pagan_fb_site_marginals_batch over FullProbability handles of one device (one launch per pass): a list of dicts as
    FullProbability.site_marginals returns."""
    L = lib()
    n = len(fbs)
    out = [{} for _ in range(n)]
    args = []
    for name, side, kind in _MARGINALS:
        if not (columns if side else rows):
            args.append(None)
            continue
        ptrs = ((_f64p if kind == "f" else _i32p) * n)()
        for k, fb in enumerate(fbs):
            a = np.zeros(fb.shape[side], np.float64 if kind == "f" else np.int32)
            out[k][name] = a
            ptrs[k] = _dp(a) if kind == "f" else _ip(a)
        args.append(ptrs)
    handles = (C.c_void_p * n)(*[fb._h for fb in fbs])
    check(L.pagan_fb_site_marginals_batch(n, handles, *args), "pagan_fb_site_marginals_batch")
    return out


def expected_counts_batch(fbs, emissions=True):
    """pagan_fb_expected_counts_batch over FullProbability handles of one device (one launch of pg_fb_counts): a list of dicts
    as FullProbability.expected_counts returns.  emissions: one switch for all pairs, or one per pair."""
    L = lib()
    n = len(fbs)
    want = [bool(emissions)] * n if isinstance(emissions, (bool, int)) else [bool(e) for e in emissions]
    assert len(want) == n
    trans = [np.zeros(12, np.float64) for _ in fbs]
    emit = [np.zeros(fb.model.n_states ** 2, np.float64) if w else None for fb, w in zip(fbs, want)]
    tp = (_f64p * n)(*[_dp(t) for t in trans])
    ep = (_f64p * n)(*[(_dp(e) if e is not None else _f64p()) for e in emit])
    handles = (C.c_void_p * n)(*[fb._h for fb in fbs])
    check(L.pagan_fb_expected_counts_batch(n, handles, tp, ep), "pagan_fb_expected_counts_batch")
    out = []
    for k, fb in enumerate(fbs):
        S = fb.model.n_states
        out.append({"trans": trans[k][:9].reshape(3, 3).copy(), "end": trans[k][9:].copy(),
                    "emit": emit[k].reshape(S, S).T.copy() if want[k] else None})      # emit[a + b * S] -> [a, b]
    return out


def fb_counts_predict_bytes(left_sites, right_sites, n_states):
    return lib().pagan_fb_counts_predict_bytes(left_sites, right_sites, n_states)


def path_cells(cols):
    """pagan_path_cells (host only): [n, 3] int32 rows (state, i, j) of the DP cell each column sits on, (-1, -1, -1) at skip columns."""
    c = np.ascontiguousarray(cols, np.int32).reshape(-1, 3)
    out = np.zeros((c.shape[0], 3), np.int32)
    check(lib().pagan_path_cells(c.ctypes.data_as(abi.colp), c.shape[0], _ip(out)), "pagan_path_cells")
    return out


def sample_uniforms(seed, node, n):
    """pagan_sample_uniforms (host only): n numbers in [0, 1), a pure function of (seed, node, index)."""
    u = np.zeros(n, np.float64)
    check(lib().pagan_sample_uniforms(int(seed) & 0xFFFFFFFFFFFFFFFF, int(node), int(n), _dp(u)), "pagan_sample_uniforms")
    return u


def sample_uniforms_path(seed, node, path, n):
    """pagan_sample_uniforms_path (host only): the stream of path `path` of node `node`'s ensemble; path 0 is sample_uniforms."""
    u = np.zeros(n, np.float64)
    check(lib().pagan_sample_uniforms_path(int(seed) & 0xFFFFFFFFFFFFFFFF, int(node), int(path), int(n), _dp(u)),
          "pagan_sample_uniforms_path")
    return u


def fb_predict_bytes(left_sites, right_sites, band=None, n_states=None):
    """pagan_fb_predict_bytes; with n_states pagan_fb_predict_bytes_states (a score table beyond 211 x 211 counted)."""
    if n_states is None:
        return lib().pagan_fb_predict_bytes(left_sites, right_sites, _band(band))
    return lib().pagan_fb_predict_bytes_states(left_sites, right_sites, _band(band), int(n_states))


def debug_far(left, right, band=None):
    """Diagnostic (host only): the far histories of a banded job -- (n_served, hfL[Lx], hfR[Ly], hbit[nd], classes[nd])."""
    L = lib()
    Lx, Ly = left.n_sites - 1, right.n_sites - 1
    nd = Lx + Ly - 1
    hfl, hfr, hb, cls = np.zeros(Lx, np.uint8), np.zeros(Ly, np.uint8), np.zeros(nd, np.uint8), np.zeros(nd, np.uint8)
    n = check(L.pagan_dp_debug_far(C.byref(left.c), C.byref(right.c), _band(band), hfl.ctypes.data_as(_u8p), hfr.ctypes.data_as(_u8p),
                                   hb.ctypes.data_as(_u8p), cls.ctypes.data_as(_u8p)), "pagan_dp_debug_far")
    return n, hfl, hfr, hb, cls


def debug_descriptors(left, right, band=None, n_states=15):
    """Diagnostic (host only): the descriptor words pg_fill_pipe would read for this job under a model of n_states states, as an
    int32 array [diagonals, 8] (include/pagan_dp.h has the layout); [0, 8] for a job the planner does not give to pg_fill_pipe."""
    nd = left.n_sites + right.n_sites - 3
    words = np.zeros((nd, 8), np.int32)
    n = check(lib().pagan_dp_debug_descriptors(C.byref(left.c), C.byref(right.c), _band(band), int(n_states), _ip(words), words.size),
              "pagan_dp_debug_descriptors")
    return words[:n]


def debug_plan(left, right, band=None, with_lead=False):
    """Diagnostic (host only): (classes[Lx+Ly-1] uint8, [awake intervals of wave 0..3]) the banded fill kernel
    would be given for this job; with_lead adds the per-diagonal downstream-progress requirement."""
    L = lib()
    nd = left.n_sites + right.n_sites - 3
    cls = np.zeros(nd, np.uint8)
    cap = 8 * nd + 64
    sched = np.zeros(cap, np.int32)
    n = C.c_int32()
    lead = np.zeros(nd, np.int32)
    check(L.pagan_dp_debug_plan(C.byref(left.c), C.byref(right.c), _band(band), cls.ctypes.data_as(_u8p), nd, _ip(sched), cap, C.byref(n),
                                _ip(lead)), "pagan_dp_debug_plan")
    waves = []
    for w in range(4):
        k = int(sched[w])
        iv = []
        while sched[k] < nd:
            iv.append((int(sched[k]), int(sched[k + 1])))
            k += 2
        waves.append(iv)
    if with_lead:
        return cls, waves, lead
    return cls, waves


class Batch(Handle):
    """Jobs uploaded once and kept resident in HBM; run() replays the hot path on them."""

    _destroy = "pagan_batch_destroy"

    def __init__(self, jobs, flags=0, device=-1):
        self._L = lib()
        self.jobs = list(jobs)          # keeps the numpy arrays alive
        self.n = len(self.jobs)
        arr = _jobs_array(self.jobs)
        opts = abi.COpts(flags, device)
        self._h = C.c_void_p()
        check(self._L.pagan_batch_create(self.n, arr, C.byref(opts), C.byref(self._h)), "pagan_batch_create")

    @property
    def cells(self):
        return self._L.pagan_batch_cells(self._h)

    def run(self):
        check(self._L.pagan_batch_run(self._h), "pagan_batch_run")

    def sync(self):
        check(self._L.pagan_batch_sync(self._h), "pagan_batch_sync")

    def last_ms(self):
        ms = (C.c_double * 2)()
        check(self._L.pagan_batch_last_ms(self._h, ms), "pagan_batch_last_ms")
        return ms[0], ms[1]

    def fetch(self):
        res = (abi.CResult * self.n)()
        rc = self._L.pagan_batch_fetch(self._h, res)
        try:
            check(rc, "pagan_batch_fetch")
            return [Result(r) for r in res]
        finally:
            for r in res:
                self._L.pagan_result_free(C.byref(r))

    def debug_scores(self, k):
        """Diagnostic: job k's device score array as [cells, 3] float64 (X, Y, M), diagonal-major."""
        out = np.empty((self.cells_of(k), 3), np.float64)
        check(self._L.pagan_batch_debug_scores(self._h, k, _dp(out), out.size), "pagan_batch_debug_scores")
        return out

    def debug_backptrs(self, k):
        """Diagnostic: job k's device back-pointer array as [cells, 3] uint32 (X, Y, M), diagonal-major."""
        out = np.empty((self.cells_of(k), 3), np.uint32)
        check(self._L.pagan_batch_debug_backptrs(self._h, k, out.ctypes.data_as(_u32p), out.size), "pagan_batch_debug_backptrs")
        return out

    def debug_followed(self, k):
        """Diagnostic: (chunks of 16 diagonals of job k whose back-pointers were written behind the banded fill by its
        follower workgroups, all chunks of the job); (0, 0) for a job of another kernel."""
        c = (C.c_int32 * 2)()
        check(self._L.pagan_batch_debug_followed(self._h, k, c), "pagan_batch_debug_followed")
        return int(c[0]), int(c[1])

    def debug_poke_bp(self, k, i, j, vit, word):
        """Test hook: after the next run's fill, state `vit` of cell (i, j) of job k gets `word` as its back-pointer (once)."""
        check(self._L.pagan_batch_debug_poke_bp(self._h, k, i, j, vit, word), "pagan_batch_debug_poke_bp")

    def debug_reruns(self):
        """How often fetch() ran the batch again after a failed path check."""
        return int(self._L.pagan_batch_debug_reruns(self._h))

    def debug_trace(self, k, n_cells):
        """Diagnostic: the first n_cells visited cells of job k's last traceback as [n, 3] int32 rows (i, j, word)."""
        out = np.empty((n_cells, 3), np.int32)
        check(self._L.pagan_batch_debug_trace(self._h, k, out.ctypes.data_as(C.c_void_p), out.nbytes), "pagan_batch_debug_trace")
        return out

    def debug_segments(self, k):
        """Diagnostic: (n_bound, [n_segments, 5] int32 rows (i, j, state, cells, offset), cells of the path, device status)
        of job k's last traceback."""
        info = np.zeros(4, np.int32)
        check(self._L.pagan_batch_debug_segments(self._h, k, _ip(info), None, 0), "pagan_batch_debug_segments")
        segs = np.zeros((int(info[1]), 5), np.int32)
        check(self._L.pagan_batch_debug_segments(self._h, k, _ip(info), _ip(segs), segs.shape[0]), "pagan_batch_debug_segments")
        return int(info[0]), segs, int(info[2]), int(info[3])

    def cells_of(self, k):
        left, right, _, band = self.jobs[k]
        return self._L.pagan_dp_count_cells(left.n_sites, right.n_sites, _band(band))
