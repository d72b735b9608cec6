"""CPU: the expected transition / emission counts -- the exact reading checks itself, the estimator, the argument errors, the
exports and the two walk setters through the batch-backend seam.  No device is needed.

The exact reading (tests/pycheck_counts.py over pycheck_fb.Exact) is what tests/test_fb_counts_gpu.py compares pg_fb_counts with;
here it is pinned from another side: each count is the derivative of log_fwd by the matching log parameter, so central
differences of the exact log_fwd under a perturbed gap_ext / gap_open / non_gap must give the count sums.  The parameters are
floats (pycheck_fb promotes them one by one), so the perturbed values are rounded to float32 first and the step is taken from the
rounded values.  Relative step 1e-3, bound 1e-5 relative.  The central difference's error is its truncation error h^2 / 6 times
the third derivative of log_fwd by the log parameter -- the third cumulant of the number of such arcs on a path, which long
gaps skew --: measured here 9.9e-6 (gap_ext), 1.2e-7 (gap_open), 1.7e-6 (non_gap) on the full pair, and a quarter of each at half
the step, as h^2 says.  The identity needs log_fwd = log_bwd (one edge at either end site): with more, the forward end corner
counts some Y-closes more than once and log_fwd's derivative weighs those paths more than the counts, which use B, do."""
import ctypes as C
import math

import numpy as np
import pytest

import pagan2_msa_amd as pgm
from pagan2_msa_amd import abi, host, synth

import pycheck_counts
import pycheck_fb
from fb_testlib import random_tunnel

BF = [0.3, 0.2, 0.2, 0.3]
STEP = 1e-3


def pair_70x66():
    """the p_dead = 0.03 pair of tests/test_fb_exact_gpu.py (its P2): one edge at either end site, so log_fwd = log_bwd and the
    forward total's derivative is the counts' sum exactly"""
    left = synth.random_graph(70, 4, 30, p_extra=0.4, max_deg=4, max_span=20, p_dead=0.03)
    right = synth.random_graph(66, 4, 530, p_extra=0.4, max_deg=4, max_span=20, p_dead=0.03)
    return left, right, host.model_prob(1, 0.1, base_freq=BF)


@pytest.fixture(scope="module")
def cases(pg):
    """{name: (left, right, mp, band, counts)}: the pair in full and behind a tunnel, the exact counts computed once"""
    left, right, mp = pair_70x66()
    band = random_tunnel(np.random.default_rng(2), left.n_sites - 1, right.n_sites - 1, 8, 30)
    return {name: (left, right, mp, b, pycheck_counts.run(left, right, mp, b)) for name, b in (("full", None), ("tunnel", band))}


@pytest.mark.parametrize("name", ["full", "tunnel"])
def test_end_counts_sum_to_one_and_arcs_sum_to_the_posterior(cases, name):
    left, right, mp, band, c = cases[name]
    ex = c["exact"]
    assert np.isfinite(ex.log_fwd) and ex.log_fwd == ex.log_bwd
    assert abs(c["end"].sum() - 1.0) <= 1e-12, c["end"]
    post = ex.posterior()
    got, want = c["trans"].sum(axis=0), post.sum(axis=(0, 1))
    want[2] -= post[0, 0, 2]                                        # (the start corner has no arc in)
    print("%s: arcs into X, Y, M %s, posterior sums %s, end %s" % (name, got, want, c["end"]))
    assert np.all(np.abs(got - want) <= 1e-12 * np.maximum(1.0, want)), (got, want)
    cellwise = post.copy()
    cellwise[0, 0, 2] = 0.0
    assert np.abs(c["into"] - cellwise).max() <= 1e-14
    # the emission table holds the M posteriors of the cells with i, j >= 1, and nothing lies on a start row or column
    assert abs(c["emit"].sum() - post[1:, 1:, 2].sum()) <= 1e-12 and post[0, 1:, 2].sum() == 0 and post[1:, 0, 2].sum() == 0


@pytest.mark.parametrize("name", ["full", "tunnel"])
def test_counts_are_the_gradient_of_log_fwd(cases, name):
    left, right, mp, band, c = cases[name]
    sums = pycheck_counts.gradient_sums(c)
    worst = {}
    for key, attr in (("ext", "gap_ext"), ("open", "gap_open"), ("ng", "non_gap")):
        v = getattr(mp, attr)
        lo, hi = float(np.float32(v * (1 - STEP))), float(np.float32(v * (1 + STEP)))
        logs = []
        for val in (lo, hi):
            p = {"gap_open": mp.gap_open, "gap_ext": mp.gap_ext, "non_gap": mp.non_gap}
            p[attr] = val
            logs.append(pycheck_fb.Exact(left, right, abi.ModelProb(mp.score, p["gap_open"], p["gap_ext"], p["non_gap"]), band).log_fwd)
        grad = (logs[1] - logs[0]) / (math.log(hi) - math.log(lo))
        worst[key] = abs(grad - sums[key]) / abs(sums[key])
        assert worst[key] <= 1e-5, (name, key, grad, sums[key])
    print("%s: central differences against the count sums, relative: %s" % (name, worst))


# ---- pagan_fit_indel ----

def node_counts_from(r, dist, n_out=1000.0, gap=(40.0, 10.0, 7.0, 3.0)):
    """trans[12] whose match-exit counts follow t = 1 - exp(-0.5 r dist) exactly: O = 2 t n, S = (1 - 2 t) n"""
    t = 1.0 - math.exp(-0.5 * r * dist)
    tr = np.zeros(12)
    tr[6] = 0.7 * 2 * t * n_out; tr[7] = 0.3 * 2 * t * n_out              # n_MX, n_MY
    tr[8] = (1 - 2 * t) * n_out - 1.0; tr[11] = 1.0                        # n_MM, n_Mend
    tr[0], tr[4] = gap[0], gap[1]                                         # n_XX, n_YY
    tr[1] = tr[3] = 0.5; tr[2] = gap[2]; tr[5] = gap[3]; tr[9] = 0.25; tr[10] = 0.75
    return tr


def test_fit_indel_one_node_is_the_closed_form(pg):
    r, d = 0.07, 0.31
    tr = node_counts_from(r, d)
    rate, ext = host.fit_indel([d], [tr])
    O, S = tr[6] + tr[7], tr[8] + tr[11]
    t = O / (2 * (O + S))
    assert abs(rate - (-math.log(1 - t) / d)) <= 1e-9 * rate          # r / 2 = -ln(1 - t) / d
    assert abs(rate - r / 2) <= 1e-9 * rate
    assert abs(ext - 50.0 / (50.0 + 1.0 + 10.0 + 1.0)) <= 1e-15


def test_fit_indel_two_nodes_recover_the_rate(pg):
    r = 0.046
    rate, ext = host.fit_indel([0.12, 0.83], [node_counts_from(r, 0.12, 700.0), node_counts_from(r, 0.83, 1900.0)])
    print("two nodes: rate %.15g, wanted %.15g" % (rate, r / 2))
    assert abs(rate - r / 2) <= 1e-9 * (r / 2)
    # dict input as Msa.node_counts gives it
    as_dict = lambda tr: {"trans": tr[:9].reshape(3, 3), "end": tr[9:]}
    assert host.fit_indel([0.12, 0.83], [as_dict(node_counts_from(r, 0.12, 700.0)), as_dict(node_counts_from(r, 0.83, 1900.0))]) == (rate, ext)


def test_fit_indel_degenerate_counts_are_defined(pg):
    """All-zero counts: rate 0, gap_ext 0.  No gap opened (O = 0): rate 0.  A node of distance 0 is left out of the rate."""
    assert host.fit_indel([0.3], [np.zeros(12)]) == (0.0, 0.0)
    assert host.fit_indel([], np.zeros((0, 12))) == (0.0, 0.0)
    tr = node_counts_from(0.05, 0.3)
    tr[6] = tr[7] = 0.0
    rate, ext = host.fit_indel([0.3], [tr])
    assert rate == 0.0 and 0 < ext < 1
    both = host.fit_indel([0.0, 0.3], [node_counts_from(0.05, 0.3), node_counts_from(0.05, 0.3)])
    assert abs(both[0] - 0.025) <= 1e-9 * 0.025
    H = host._lib()
    bad = node_counts_from(0.05, 0.3)
    bad[4] = -1.0
    f64p = C.POINTER(C.c_double)
    a, b = C.c_double(), C.c_double()
    d = np.array([0.3])
    assert H.pagan_fit_indel(1, d.ctypes.data_as(f64p), bad.ctypes.data_as(f64p), C.byref(a), C.byref(b)) == abi.PAGAN_E_ARG
    assert H.pagan_fit_indel(1, d.ctypes.data_as(f64p), None, C.byref(a), C.byref(b)) == abi.PAGAN_E_ARG
    assert H.pagan_fit_indel(1, d.ctypes.data_as(f64p), bad.ctypes.data_as(f64p), None, C.byref(b)) == abi.PAGAN_E_ARG


# ---- exports and argument errors ----

NEW_DP = ["pagan_fb_expected_counts", "pagan_fb_expected_counts_batch", "pagan_fb_counts_ms", "pagan_fb_counts_predict_bytes"]
NEW_HOST = ["pagan_msa_set_counts", "pagan_msa_node_counts", "pagan_msa_set_indel_model", "pagan_fit_indel"]


def test_new_symbols_are_exported_and_refuse_bad_arguments_without_a_device(pg):
    lib = C.CDLL(pgm.LIB_PATH)
    for sym in NEW_DP:
        assert sym in abi.EXPORTED and getattr(lib, sym) is not None
    for sym in NEW_HOST:
        assert sym in host.HOST_EXPORTED and getattr(lib, sym) is not None
    L = pgm.lib()
    f64p = C.POINTER(C.c_double)
    trans = np.zeros(12)
    tp = (f64p * 1)(trans.ctypes.data_as(f64p))
    assert L.pagan_fb_expected_counts(None, trans.ctypes.data_as(f64p), None) == abi.PAGAN_E_ARG
    assert L.pagan_fb_expected_counts_batch(1, None, tp, None) == abi.PAGAN_E_ARG
    assert L.pagan_fb_expected_counts_batch(1, (C.c_void_p * 1)(None), tp, None) == abi.PAGAN_E_ARG     # a NULL handle
    assert L.pagan_fb_expected_counts_batch(-1, None, None, None) == abi.PAGAN_E_ARG
    assert L.pagan_fb_expected_counts_batch(0, None, None, None) == abi.PAGAN_OK
    assert L.pagan_fb_counts_ms(None, None) == abi.PAGAN_E_ARG
    # the scratch: per work item (a row block of 64 rows x a segment of 256 diagonals) 8 B an entry and 12 B of the item; the
    # emission table only up to 32 states
    small, big = pgm.fb_counts_predict_bytes(71, 67, 15), pgm.fb_counts_predict_bytes(641, 67, 15)
    assert big - small == (8 * (9 + 225) + 12) * (10 - 2)
    assert pgm.fb_counts_predict_bytes(641, 67, 211) - pgm.fb_counts_predict_bytes(71, 67, 211) == (8 * 9 + 12) * 8
    assert pgm.fb_counts_predict_bytes(71, 2001, 15) - small == (8 * (9 + 225) + 12) * 2 * (9 - 1)       # 2,063 diagonals: 9 segments
    assert pgm.fb_counts_predict_bytes(1, 67, 15) == abi.PAGAN_E_ARG
    H = host._lib()
    assert H.pagan_msa_set_counts(None, 1) == abi.PAGAN_E_ARG
    assert H.pagan_msa_node_counts(None, 0, None, None) == abi.PAGAN_E_ARG
    assert H.pagan_msa_set_indel_model(None, 0.01, 0.01, 0.5, 0.5) == abi.PAGAN_E_ARG


# ---- the walk's setters through the batch-backend seam ----

def recording_backend(oracle, seen):
    L = oracle.lib()

    def fn(n, jobs, opts, out, user):
        for k in range(n):
            j = jobs[k]
            m = j.model.contents
            seen.append(tuple(np.float32(v) for v in (m.log_gap_open, m.log_gap_ext, m.log_gap_end_ext, m.log_non_gap)))
            rc = L.oracle_dp_align(j.left, j.right, j.model, j.band if j.band else None, opts, C.byref(out[k]))
            if rc != 0:
                return rc
        return 0
    return fn


def model_params(ins, dele, ext, end_ext, dist):
    """ModelFactory::alignment_model's float expressions: (log_gap_open, log_gap_ext, log_gap_end_ext, log_non_gap)"""
    rate = np.float32(ins) + np.float32(dele)                       # float + float
    t = 1.0 - math.exp(-0.5 * float(rate) * dist)
    lg = lambda x: np.float32(math.log(float(np.float32(x))))
    return (np.float32(math.log(t)), lg(ext), lg(end_ext), np.float32(math.log(1.0 - 2 * t)))


def walk_params(oracle, names, seqs, nwk, **kw):
    seen = []
    msa = host.Msa(names, seqs, nwk, use_anchors=0, **kw)
    msa.set_batch_backend(recording_backend(oracle, seen))
    msa.align()
    per_node = []
    for k in range(msa.n_internal):
        m = msa.node_cjob(k).model.contents
        per_node.append((msa.node_info(k).dist, tuple(np.float32(v) for v in (m.log_gap_open, m.log_gap_ext, m.log_gap_end_ext, m.log_non_gap))))
    return msa, seen, per_node


def test_set_indel_model_reaches_the_backend_at_every_node(pg, oracle):
    names, seqs, _ = synth.evolve_balanced(4, 60, branch=0.05, sub=0.05, indel_start=0.01, mean_len=3, seed=21)
    nwk = "((S000:0.05,S001:0.09):0.03,(S002:0.02,S003:0.11):0.07);"      # three node distances: 0.14, 0.13, 0.10
    DNA = (0.01, 0.01, 0.8, 0.95)                                   # the data type's defaults
    for arg, eff in (((0.03, 0.05, 0.6, 0.9), (0.03, 0.05, 0.6, 0.9)),
                     ((-1, 0.04, -1, 0.5), (0.01, 0.04, 0.8, 0.5)),
                     ((-1, -1, -1, -1), DNA), (None, DNA)):
        msa, seen, per_node = walk_params(oracle, names, seqs, nwk, indel_model=arg)
        dists = {d for d, _ in per_node}
        assert len(dists) == 3
        for dist, got in per_node:
            want = model_params(*eff, dist)
            assert got == want, (arg, dist, got, want)
        assert sorted(seen) == sorted(p for _, p in per_node), arg  # what the backend received is what the nodes record
    # the unset walk and the all-negative one give the same alignment
    a = walk_params(oracle, names, seqs, nwk)[0].alignment_all()
    assert walk_params(oracle, names, seqs, nwk, indel_model=(-1, -1, -1, -1))[0].alignment_all() == a


def test_set_indel_model_refuses_what_cannot_be_a_model(pg, oracle):
    names, seqs, nwk = synth.evolve_balanced(4, 40, branch=0.05, sub=0.05, indel_start=0.01, mean_len=3, seed=22)
    H = host._lib()
    msa = host.Msa(names, seqs, nwk, use_anchors=0)
    for bad in ((0.01, 0.01, 1.0, 0.5), (0.01, 0.01, 0.5, 0.0), (float("nan"), 0.01, 0.5, 0.5), (0.0, 0.0, 0.5, 0.5)):
        assert H.pagan_msa_set_indel_model(msa._h, *bad) == abi.PAGAN_E_ARG, bad
    # rates that leave no room for a match at some node's distance: refused at align time
    far = host.Msa(names, seqs, nwk, use_anchors=0, indel_model=(8.0, 8.0, -1, -1))
    far.set_batch_backend(recording_backend(oracle, []))
    with pytest.raises(pgm.PaganError) as e:
        far.align()
    assert e.value.code == abi.PAGAN_E_ARG
    with pytest.raises(pgm.PaganError) as e:
        far.align_nodes(far.ready()[:1])
    assert e.value.code == abi.PAGAN_E_ARG
    # after a round has run the model is fixed
    msa.set_batch_backend(recording_backend(oracle, []))
    msa.align_nodes(msa.ready()[:1])
    assert H.pagan_msa_set_indel_model(msa._h, 0.02, 0.02, 0.5, 0.5) == abi.PAGAN_E_ARG


def test_set_counts_without_a_pass_is_an_argument_error(pg, oracle):
    names, seqs, nwk = synth.evolve_balanced(4, 40, branch=0.05, sub=0.05, indel_start=0.01, mean_len=3, seed=22)
    msa = host.Msa(names, seqs, nwk, use_anchors=0, expected_counts=1)
    msa.set_batch_backend(recording_backend(oracle, []))
    with pytest.raises(pgm.PaganError) as e:
        msa.align()
    assert e.value.code == abi.PAGAN_E_ARG
    with pytest.raises(pgm.PaganError) as e:
        msa.align_nodes(msa.ready()[:1])
    assert e.value.code == abi.PAGAN_E_ARG
    assert host._lib().pagan_msa_set_counts(msa._h, 2) == abi.PAGAN_E_ARG
    # with a pass asked for, the seam has none: the walk fails loudly instead of skipping the counts
    withfb = host.Msa(names, seqs, nwk, use_anchors=0, expected_counts=1, full_probability=1)
    withfb.set_batch_backend(recording_backend(oracle, []))
    with pytest.raises(pgm.PaganError) as e:
        withfb.align()
    assert e.value.code == abi.PAGAN_E_NODEVICE
    # a walk without counts keeps none
    plain = host.Msa(names, seqs, nwk, use_anchors=0)
    plain.set_batch_backend(recording_backend(oracle, []))
    plain.align()
    with pytest.raises(pgm.PaganError) as e:
        plain.node_counts(0)
    assert e.value.code == abi.PAGAN_E_ARG
    assert [f[0] for f in host.CMsaOpts._fields_][-3:] == ["full_probability", "sample_path", "sample_seed"]
