"""CPU: posterior decoding without a device -- the definition pinned by a hand-worked vector and by brute force over every path of
tiny pairs (tests/pycheck_mea.py), the route decided in fb_decode_route, the size prediction, the new entry points, the tree walk's
decoder switch behind the test seam, and the code-object metadata of the ring and trace kernels (no scratch, no spill: a spilled
register would put a memory round trip of its own on a step that exists to have none)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import pagan2_msa_amd as pgm
from pagan2_msa_amd import abi, host, synth

import pycheck_fb
import pycheck_mea
from fb_testlib import random_tunnel
from pycheck_fb import X, Y, M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pagan2-msa_amd", "csrc")
BF = [0.3, 0.2, 0.2, 0.3]
NINF = float("-inf")


def test_hand_worked_two_residues_a_side():
    """Two plain sequences of two residues: 3 x 3 cells (site 0 is the start site), every cell one predecessor per state.
    A made-up posterior table, g = 0.5 -- weights w = posterior (M), posterior / 2 (X, Y):

        w_X: (1,0) .2  (2,0) .1  (2,1) .15 (2,2) .05       w_Y: (0,1) .2  (0,2) .1  (1,2) .4  (2,2) .05
        w_M: (1,1) .6  (1,2) .1  (2,1) .2  (2,2) .7        everything else 0

    A, cell by cell (X reads (i-1, j) as X, Y, M; Y reads (i, j-1) as Y, X, M; M reads (i-1, j-1) as M, X, Y):

        (0,0) M 0                      (0,1) Y 0+.2 = .2              (0,2) Y .2+.1 = .3
        (1,0) X 0+.2 = .2              (2,0) X .2+.1 = .3
        (1,1) X .2+0 = .2 (from Y(0,1))   Y .2+0 = .2 (from X(1,0))   M 0+.6 = .6
        (1,2) X .3+0 = .3 (from Y(0,2))   Y .6+.4 = 1.0 (from M(1,1)) M .2+.1 = .3 (from Y(0,1))
        (2,1) X .6+.15 = .75 (from M(1,1))  Y .3+0 = .3 (from X(2,0)) M .2+.2 = .4 (from X(1,0))
        (2,2) X 1.0+.05 = 1.05 (from Y(1,2))  Y .75+.05 = .8 (from X(2,1))  M .6+.7 = 1.3 (from M(1,1))

    End: M(2,2) 1.3, X(2,2) 1.05, Y(2,2) .8 -> objective 1.3 along M(2,2), M(1,1)."""
    left, right = synth.chain_graph("AC"), synth.chain_graph("AG")
    assert left.n_sites == 4 and right.n_sites == 4
    ex = pycheck_fb.Exact(left, right, host.model_prob(1, 0.1, base_freq=BF))
    post = np.zeros((3, 3, 3))
    for (i, j), p in {(1, 0): .4, (2, 0): .2, (2, 1): .3, (2, 2): .1}.items():
        post[i, j, X] = p
    for (i, j), p in {(0, 1): .4, (0, 2): .2, (1, 2): .8, (2, 2): .1}.items():
        post[i, j, Y] = p
    for (i, j), p in {(1, 1): .6, (1, 2): .1, (2, 1): .2, (2, 2): .7}.items():
        post[i, j, M] = p
    mea = pycheck_mea.Mea(ex, post, 0.5)
    want = np.full((3, 3, 3), NINF)
    want[0, 0, M] = 0
    want[0, 1, Y], want[0, 2, Y], want[1, 0, X], want[2, 0, X] = .2, .3, .2, .3
    want[1, 1] = (.2, .2, .6)
    want[1, 2] = (.3, 1.0, .3)
    want[2, 1] = (.75, .3, .4)
    want[2, 2] = (1.05, .8, 1.3)
    assert np.array_equal(np.isfinite(mea.A), np.isfinite(want))
    fin = np.isfinite(want)
    assert np.allclose(mea.A[fin], want[fin], rtol=0, atol=1e-15)
    assert mea.status == 0 and abs(mea.objective - 1.3) <= 1e-15 and mea.end == (M, 2, 2)
    assert mea.visited.tolist() == [[2, 2, M], [1, 1, M]]
    assert pycheck_mea.is_path(ex, mea.visited, mea.end)
    assert not pycheck_mea.is_path(ex, [[2, 2, M], [1, 2, Y]], mea.end)          # (a match does not follow a cell of its own row)
    assert abs(pycheck_mea.objective_of(mea.w, mea.visited) - 1.3) <= 1e-15
    best, n_paths = pycheck_mea.brute_force(ex, post, 0.5)
    assert abs(best - 1.3) <= 1e-15 and n_paths > 10
    # the gap weight decides: with gaps counted four-fold the path leaves the diagonal
    heavy = pycheck_mea.Mea(ex, post, 2.0)
    assert abs(heavy.objective - pycheck_mea.brute_force(ex, post, 2.0)[0]) <= 1e-12
    assert heavy.objective > 2.0 and heavy.visited.tolist() != mea.visited.tolist()


def tiny_pairs():
    """(name, left, right, band): 36 pairs of at most 5 sites a side -- every third behind a band, every other with dead sites"""
    out = []
    for k in range(36):
        rng = np.random.default_rng(900 + k)
        nl, nr = int(rng.integers(1, 4)), int(rng.integers(1, 4))
        p_dead = 0.3 if k % 2 else 0.0
        left = synth.random_graph(nl, 4, 2 * k, p_extra=0.6, max_deg=3, max_span=3, p_dead=p_dead)
        right = synth.random_graph(nr, 4, 2 * k + 1, p_extra=0.6, max_deg=3, max_span=3, p_dead=p_dead)
        assert left.n_sites <= 5 and right.n_sites <= 5
        band = random_tunnel(rng, left.n_sites - 1, right.n_sites - 1, 1, 3) if k % 3 == 0 else None
        out.append(("T%d" % k, left, right, band))
    return out


def test_the_fill_equals_brute_force_on_tiny_pairs():
    mp = host.model_prob(1, 0.3, base_freq=BF)
    n_finite = n_zero = n_paths_all = 0
    for name, left, right, band in tiny_pairs():
        ex = pycheck_fb.Exact(left, right, mp, band)
        post = ex.posterior()
        logf = ex.log_f()
        for g in (0.0, 0.5, 1.0):
            mea = pycheck_mea.Mea(ex, post, g)
            best, n_paths = pycheck_mea.brute_force(ex, post, g)
            # A is finite exactly where the forward matrix is
            assert np.array_equal(np.isfinite(mea.A), np.isfinite(logf)), (name, g)
            if best is None:
                assert mea.status == 1 and mea.objective == 0.0 and len(mea.visited) == 0 and ex.log_fwd == NINF, (name, g)
                n_zero += 1
                continue
            n_finite += 1
            n_paths_all += n_paths
            assert mea.status == 0 and np.isfinite(ex.log_fwd), (name, g)
            assert abs(mea.objective - best) <= 1e-12, (name, g, mea.objective, best)
            assert pycheck_mea.is_path(ex, mea.visited, mea.end), (name, g)
            assert abs(pycheck_mea.objective_of(mea.w, mea.visited) - mea.objective) <= 1e-12, (name, g)
    assert n_finite >= 3 * 30 and n_paths_all > 1000, (n_finite, n_zero, n_paths_all)


def plain(n, seed):
    rng = np.random.default_rng(seed)
    return synth.chain_graph("".join(rng.choice(list("ACGT"), n)))


def test_route_without_a_device(pg, monkeypatch):
    monkeypatch.delenv("PAGAN_FB_DECODE_RING", raising=False)
    a, b = plain(40, 1), plain(37, 2)
    band = random_tunnel(np.random.default_rng(3), a.n_sites - 1, b.n_sites - 1, 4, 9)
    assert pgm.fb_decode_route(a, b) == 1 and pgm.fb_decode_route(a, b, band) == 1
    # whichever schedule the sweeps take: the forward/backward switches do not move the decode
    monkeypatch.setenv("PAGAN_FB_RING", "0")
    assert pgm.fb_decode_route(a, b, band) == 1
    monkeypatch.delenv("PAGAN_FB_RING")
    graph = synth.random_graph(40, 4, 5, p_extra=0.4, max_deg=4, max_span=6)
    assert pgm.fb_decode_route(graph, b) == 0 and pgm.fb_decode_route(a, graph, None) == 0
    wide_a, wide_b = plain(1100, 6), plain(1090, 7)
    assert pgm.fb_decode_route(wide_a, wide_b) == 0                               # a diagonal of more than 1,024 cells
    tunnel = random_tunnel(np.random.default_rng(8), wide_a.n_sites - 1, wide_b.n_sites - 1, 8, 30)
    assert pgm.fb_decode_route(wide_a, wide_b, tunnel) == 1
    monkeypatch.setenv("PAGAN_FB_DECODE_RING", "0")
    assert pgm.fb_decode_route(a, b) == 0 and pgm.fb_decode_route(wide_a, wide_b, tunnel) == 0
    monkeypatch.setenv("PAGAN_FB_DECODE_RING", "1")
    assert pgm.fb_decode_route(a, b) == 1
    assert pgm.lib().pagan_fb_debug_decode_route(None, C.byref(b.c), None) == abi.PAGAN_E_ARG


def test_predict_bytes_grows_by_24_bytes_a_cell(pg):
    L = pgm.lib()
    for lx, ly in ((301, 281), (72, 68), (2001, 1901)):
        cells = L.pagan_dp_count_cells(lx, ly, None)
        need = pgm.fb_decode_predict_bytes(lx, ly)
        assert 24 * cells + 12 * (lx + ly - 2) <= need <= 24 * cells * 17 // 16 + 12 * (lx + ly) + 8192
        band = random_tunnel(np.random.default_rng(lx), lx - 1, ly - 1, 8, 30)
        in_band = L.pagan_dp_count_cells(lx, ly, C.byref(band.c))
        banded = pgm.fb_decode_predict_bytes(lx, ly, band)
        assert in_band < cells and 24 * in_band <= banded <= 24 * in_band * 17 // 16 + 12 * (lx + ly) + 8192
        # the difference between two bands of one pair is 24 B (and the pool's sixteenth) a cell
        assert abs((need - banded) - 24 * (cells - in_band) * 17 / 16) <= 16
    assert pgm.fb_decode_predict_bytes(1, 5) < 0


# (left_sites, right_sites, band half-width or None) -> pagan_fb_predict_bytes, pagan_fb_decode_predict_bytes,
# pagan_fb_sample_predict_bytes for (n_paths, traces) = (1, on), (1, off), (65, on), (65, off), pagan_fb_counts_predict_bytes for
# S = 15, 211.  The literals were recorded by running the library of the commit before the readers' sizes came from one
# function each: the predictors' values are part of the interface (the walk cuts its sub-batches by them).
PINNED_BYTES = [
    ((2, 2, None), 566240, 1889, (1864, 1608, 7752, 5704), (5380, 1780)),
    ((301, 281, None), 4921427, 2150776, (8776, 1608, 465480, 5704), (22336, 2536)),
    ((1001, 11, None), 1200425, 268896, (13896, 1608, 805960, 5704), (33640, 3040)),
    ((301, 281, 12), 1011359, 195742, (8776, 1608, 465480, 5704), (22336, 2536)),
]


def test_the_predictors_values_are_pinned(pg):
    for (lx, ly, half), fb, decode, sample, counts in PINNED_BYTES:
        band = None
        if half is not None:                                                      # a band of constant half-width about the diagonal
            centre = np.arange(lx - 1) * (ly - 2) // (lx - 2)
            band = abi.Band(np.maximum(centre - half, 0).astype(np.int32), np.minimum(centre + half, ly - 2).astype(np.int32))
        what = (lx, ly, half)
        assert pgm.fb_predict_bytes(lx, ly, band) == fb, what
        assert pgm.fb_decode_predict_bytes(lx, ly, band) == decode, what
        got = tuple(pgm.fb_sample_predict_bytes(lx, ly, k, traces=t) for k in (1, 65) for t in (True, False))
        assert got == sample, (what, got)
        assert tuple(pgm.fb_counts_predict_bytes(lx, ly, s) for s in (15, 211)) == counts, what


def test_the_predictor_with_states_adds_the_table_beyond_211(pg):
    """pagan_fb_predict_bytes_states: the pinned function's value up to 211 states, beyond that 17/16 of what 8 S^2 exceeds the
    protein table's 8 * 211^2 by; the codon pair of test_fb_gpu.py (41 x 40 sites) comes out above its table alone."""
    for (lx, ly, half), fb, _decode, _sample, _counts in PINNED_BYTES[:3]:
        for S in (1, 15, 211):
            assert pgm.fb_predict_bytes(lx, ly, None, n_states=S) == fb, (lx, ly, S)
        for S in (212, 1892):
            more = 8 * S * S - 8 * 211 * 211
            assert pgm.fb_predict_bytes(lx, ly, None, n_states=S) == fb + more + more // 16, (lx, ly, S)
    assert pgm.fb_predict_bytes(41, 40, None, n_states=1892) > 8 * 1892 * 1892 * 17 // 16
    assert pgm.fb_predict_bytes(41, 40, None, n_states=0) == abi.PAGAN_E_ARG
    assert pgm.fb_predict_bytes(1, 5, None, n_states=15) < 0
    assert pgm.lib().pagan_fb_device_bytes(None, None) == abi.PAGAN_E_ARG


def test_the_reading_uses_the_table_as_left_state_by_right_state():
    """4 x 4 protein residues under an asymmetric table with zeros (fb_tables.py): the second reading, held to brute force over
    every path, takes score[left state, right state].  The pair is made so that the transposed table gives another optimum: the
    residues at (1, 1) are (a, b) with score[a, b] = 0 < score[b, a], those at (2, 2) the other way round."""
    import fb_tables
    prot, prot_z = fb_tables.protein_tables()
    z = prot_z.score
    a, b = next((a, b) for a in range(20) for b in range(20) if a != b and z[a, b] == 0 and z[b, a] > 0)
    leaf_alpha, _ = host.alphabets(2)
    letter = lambda s: leaf_alpha[s]
    others = [s for s in range(20) if s not in (a, b)]
    ls, rs = [a, b, others[0], others[1]], [b, a, others[0], others[1]]
    left, right = (host.HGraph.leaf("".join(letter(s) for s in q), leaf_alpha).flatten() for q in (ls, rs))
    assert list(left.state[1:-1]) == ls and list(right.state[1:-1]) == rs
    flipped = abi.ModelProb(z.T.copy(), prot_z.gap_open, prot_z.gap_ext, prot_z.non_gap)
    got = {}
    for name, mp in (("as it is", prot_z), ("transposed", flipped)):
        ex = pycheck_fb.Exact(left, right, mp)
        post = ex.posterior()
        mea = pycheck_mea.Mea(ex, post, 0.5)
        best, n_paths = pycheck_mea.brute_force(ex, post, 0.5)
        assert mea.status == 0 and n_paths > 100 and abs(mea.objective - best) <= 1e-12
        got[name] = (mea, post)
    (m1, p1), (m2, p2) = got["as it is"], got["transposed"]
    assert p1[1, 1, M] == 0 and np.isneginf(m1.A[1, 1, M]) and p1[2, 2, M] > 0 and np.isfinite(m1.A[2, 2, M])
    assert p2[1, 1, M] > 0 and np.isfinite(m2.A[1, 1, M]) and p2[2, 2, M] == 0 and np.isneginf(m2.A[2, 2, M])
    assert abs(m1.objective - m2.objective) > 1e-6
    # a fill that looks no entry up at all reaches no other optimum (fb_tables.zeros_bite says why): it is the matrix that differs
    blind = pycheck_mea.Mea(pycheck_mea.exact_arcs(left, right, prot), p1, 0.5)
    assert blind.objective == m1.objective and np.isfinite(blind.A[1, 1, M])


def test_the_table_builders_conditions_hold(oracle):
    """tests/fb_tables.py without a device: the tables are asymmetric and have one-sided zeros (the builders assert it), every
    leaf pair has the width its decode instance needs, the graph and codon pairs build, the host's codon table is the oracle's,
    and the zeros decide the matrix on the two cheapest zero-table pairs (the wider ones are held to the same condition by
    test_mea_gpu.py's fixture).  R1024z: a 1,024-entry window would serve wrong states, the 2,048 of the 1,024-thread instance
    none; the 513-wide pairs would not tell the two apart."""
    import fb_tables
    leaves = fb_tables.leaf_pairs()
    shapes = fb_tables.check_shapes(leaves)
    assert {v[2] for v in shapes.values()} == {64, 512, 1024}
    pairs = dict(leaves, **fb_tables.graph_pairs())
    k = fb_tables.codon_leaf_pair(oracle)
    assert k.mp.n_states == 1892 and not np.array_equal(k.mp.score, k.mp.score.T)
    for name in ("Q64z", "G211z"):
        p = pairs[name]
        if name == "G211z":
            ex = pycheck_fb.Exact(*p.args())
            post = ex.posterior()
        else:
            ex = pycheck_mea.exact_arcs(*p.args())
            lf, _lb, post, _logf = oracle.fb(p.left, p.right, p.mp, band=p.band)
            assert np.isfinite(lf)
        mea = pycheck_mea.Mea(ex, post, 0.5)
        assert mea.status == 0
        counts = fb_tables.zeros_bite(p, pycheck_mea.exact_arcs(p.left, p.right, p.before, p.band), mea)
        assert min(counts) >= 1
        # the objective is NOT what the zeros move, behind a band and on graphs as little as in a full matrix of two sequences
        blind = pycheck_mea.Mea(pycheck_mea.exact_arcs(p.left, p.right, p.before, p.band), post, 0.5)
        assert abs(blind.objective - mea.objective) <= fb_tables.bound(mea.objective, mea.visited.shape[0] + 1), name
    w = fb_tables.wide_zero_pair()
    assert (w.Lx, w.Ly) == (1024, 1300) and fb_tables.widest_diagonal(w)[0] == 1024
    assert fb_tables.stale_window_cells(w.Lx, w.Ly, 1024) > 10000 and fb_tables.stale_window_cells(w.Lx, w.Ly, 2048) == 0
    for name in ("R513z", "Q513z"):
        assert fb_tables.stale_window_cells(leaves[name].Lx, leaves[name].Ly, 1024) == 0


NEW_DP = ["pagan_fb_decode_batch","pagan_fb_decode", "pagan_fb_decoded_summary", "pagan_fb_decoded_visited", "pagan_fb_decoded_result",
          "pagan_fb_decoded_dump", "pagan_fb_decoded_ms", "pagan_fb_debug_decode_route", "pagan_fb_decode_predict_bytes",
          "pagan_fb_decoded_destroy"]


def test_new_symbols_are_exported_and_resolve(pg):
    lib = C.CDLL(pgm.LIB_PATH)
    for sym in NEW_DP:
        assert sym in abi.EXPORTED and getattr(lib, sym) is not None
    for sym in ("pagan_msa_set_decoder", "pagan_msa_node_decode"):
        assert sym in host.HOST_EXPORTED and getattr(lib, sym) is not None
    # the calls refuse bad arguments before they look for a device
    L = pgm.lib()
    out = C.c_void_p()
    assert L.pagan_fb_decode(None, 0.5, 0, C.byref(out)) == abi.PAGAN_E_ARG
    assert L.pagan_fb_decode_batch(1, None, 0.5, 0, C.byref(out)) == abi.PAGAN_E_ARG
    assert L.pagan_fb_decode_batch(0, None, -1.0, 0, None) == abi.PAGAN_E_ARG
    assert L.pagan_fb_decode_batch(0, None, float("nan"), 0, None) == abi.PAGAN_E_ARG
    assert L.pagan_fb_decode_batch(0, None, float("inf"), 0, None) == abi.PAGAN_E_ARG
    assert L.pagan_fb_decode_batch(0, None, 0.5, 2, None) == abi.PAGAN_E_ARG                       # an unknown flag
    assert L.pagan_fb_decode_batch(0, None, 0.5, abi.DECODE_KEEP_MATRIX, None) == abi.PAGAN_OK
    assert L.pagan_fb_decoded_summary(None, None, None, None, None, None) == abi.PAGAN_E_ARG
    assert L.pagan_fb_decoded_visited(None, None, None) == abi.PAGAN_E_ARG
    assert L.pagan_fb_decoded_result(None, None) == abi.PAGAN_E_ARG
    assert L.pagan_fb_decoded_dump(None, None) == abi.PAGAN_E_ARG
    assert L.pagan_fb_decoded_ms(None, None) == abi.PAGAN_E_ARG
    L.pagan_fb_decoded_destroy(None)
    H = host._lib()
    assert H.pagan_msa_set_decoder(None, 1, 0.5) == abi.PAGAN_E_ARG
    assert H.pagan_msa_node_decode(None, 0, None) == abi.PAGAN_E_ARG


def _oracle_backend(oracle):
    L = oracle.lib()

    def fn(n, jobs, opts, out, user):
        for k in range(n):
            j = jobs[k]
            rc = L.oracle_dp_align(j.left, j.right, j.model, j.band if j.band else None, opts, C.byref(out[k]))
            if rc != 0:
                return rc
        return 0
    return fn


def test_the_seam_refuses_a_decoded_walk(pg, oracle):
    names, seqs, nwk = synth.evolve_balanced(4, 60, branch=0.03, sub=0.03, indel_start=0.01, mean_len=3, seed=12)
    msa = host.Msa(names, seqs, nwk, use_anchors=0, posterior_decode=1)
    msa.set_batch_backend(_oracle_backend(oracle))
    with pytest.raises(pgm.PaganError) as e:
        msa.align()
    assert e.value.code == abi.PAGAN_E_NODEVICE
    with pytest.raises(pgm.PaganError) as e:
        msa.align_nodes(msa.ready()[:1])
    assert e.value.code == abi.PAGAN_E_NODEVICE
    # a decoded and a sampled path at once: refused before anything runs
    both = host.Msa(names, seqs, nwk, use_anchors=0, posterior_decode=1, sample_path=1)
    both.set_batch_backend(_oracle_backend(oracle))
    with pytest.raises(pgm.PaganError) as e:
        both.align()
    assert e.value.code == abi.PAGAN_E_ARG
    # the switch off changes nothing, and nothing was decoded
    plain_ = host.Msa(names, seqs, nwk, use_anchors=0, posterior_decode=0)
    plain_.set_batch_backend(_oracle_backend(oracle))
    ref = host.Msa(names, seqs, nwk, use_anchors=0)
    ref.set_batch_backend(_oracle_backend(oracle))
    assert plain_.align().alignment_all() == ref.align().alignment_all()
    with pytest.raises(pgm.PaganError) as e:
        plain_.node_decode(0)
    assert e.value.code == abi.PAGAN_E_ARG
    H = host._lib()
    for on, g in ((2, 0.5), (1, -0.5), (1, float("nan")), (1, float("inf"))):
        assert H.pagan_msa_set_decoder(plain_._h, on, g) == abi.PAGAN_E_ARG
    # the options struct has not grown: the switch is a setter
    assert [f[0] for f in host.CMsaOpts._fields_][-3:] == ["full_probability", "sample_path", "sample_seed"]


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    out = str(tmp_path_factory.mktemp("fbdecode") / "dp_fb.s")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "--offload-device-only", "-S", "-o", out, "dp_fb.hip"],
                   check=True, cwd=CSRC, stderr=subprocess.DEVNULL)
    return open(out).read()


@pytest.mark.parametrize("kernel, instances", [("pg_fb_ring_decode", 4), ("pg_fb_decode_trace", 1)])
def test_ring_and_trace_have_no_scratch_and_no_spill(asm, kernel, instances):
    """The kernels as the build compiles them, read from the code object's metadata: no private segment, no spilled register."""
    meta = re.findall(r"\.name:\s+(\S*%s[EI]\S*)\s+\.private_segment_fixed_size:\s+(\d+)" % kernel, asm)
    assert len(meta) == instances and all(int(m[1]) == 0 for m in meta), meta
    for name, _ in meta:
        at = re.search(r"\.name:\s+" + re.escape(name) + r"\s", asm).start()
        block = asm[at:asm.index(".wavefront_size", at)]
        spills = dict(re.findall(r"\.(sgpr_spill_count|vgpr_spill_count):\s+(\d+)", block))
        assert spills == {"sgpr_spill_count": "0", "vgpr_spill_count": "0"}, (name, spills)
