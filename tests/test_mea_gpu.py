"""GPU: posterior decoding (dp_fb_decode.inc: pg_fb_decode_fill, pg_fb_ring_decode, pg_fb_decode_trace) against its second reading
(tests/pycheck_mea.py) on reference posteriors -- the exact reading's (pycheck_fb, 50-digit decimals) for the 71 x 67 pairs of
test_fb_exact_gpu.build_pairs(), the oracle's (pinned to the exact reading by test_pycheck_fb_cpu.py) for the larger plain pairs.

Tolerances derive from the project's posterior tolerance, 1e-7 relative + 1e-12 absolute a cell (test_fb_exact_gpu.py): a score
A(s, i, j) is a sum of at most i + j + 1 weights, each a posterior times a factor <= 1 here, and a maximum moves by no more than
its candidates do, so |A_dev - A_ref| <= 1e-7 |A_ref| + 1e-12 (i + j + 1); the objective the same with the path's steps.  Paths
are NOT compared cell for cell -- two candidates within rounding of one another may legitimately break differently --: the device's
path must be a path of the reference's graph, and its sum over the REFERENCE weights must reach the reference optimum to the bound.

The references (exact sums, the second reading's fills) are computed once per module."""
import ctypes as C

import numpy as np
import pytest

import pagan2_msa_amd as pgm
from pagan2_msa_amd import abi, host, synth

import fb_tables
import pycheck_fb
import pycheck_mea
import test_fb_exact_gpu as fx
from fb_tables import widest_diagonal
from fb_testlib import random_tunnel

pytestmark = pytest.mark.gpu
BF = fx.BF
DECODE_ENV = "PAGAN_FB_DECODE_RING"


def bound(ref, n):
    return 1e-7 * np.abs(ref) + 1e-12 * n


class Case:
    """A pair, its arc listing, its reference posterior, and the second reading's fill per gap weight (computed on first use)."""

    def __init__(self, p, ex, post):
        self.p, self.ex, self.post, self._mea = p, ex, post, {}

    def mea(self, g):
        if g not in self._mea:
            self._mea[g] = pycheck_mea.Mea(self.ex, self.post, g)
        return self._mea[g]


@pytest.fixture(scope="module")
def cases(pg, oracle):
    out = {}
    for name, p in fx.build_pairs().items():
        ex = pycheck_fb.Exact(*p.args())
        out[name] = Case(p, ex, ex.posterior())
    # P5z: P5t's sequences under a model whose mismatches have probability 0 -- a match step must look at the transition itself
    p5 = out["P5t"].p
    score = p5.mp.score.copy()
    score[:4, :4] = np.where(np.eye(4, dtype=bool), score[:4, :4], 0.0)
    mpz = abi.ModelProb(score, p5.mp.gap_open, p5.mp.gap_ext, p5.mp.non_gap)
    pz = fx.Pair("P5z", p5.left, p5.right, mpz, p5.band, p5.model)
    ex = pycheck_fb.Exact(*pz.args())
    out["P5z"] = Case(pz, ex, ex.posterior())
    # the ring's own shapes: ~300 x 290 residues behind a narrow tunnel (B = 64, more than 512 diagonals: two window refills),
    # behind halves (40, 70) -- whose diagonals turn out to hold 63 cells at most: a full wave, still one -- and behind halves
    # (100, 140): diagonals wider than 128 cells, four waves, the x - 1 neighbour crosses a wave
    _, seqs, _ = synth.evolve_balanced(2, 300, branch=0.1, sub=0.1, indel_start=0.02, mean_len=3, seed=21)
    gl, gr = (host.HGraph.leaf(s).flatten() for s in seqs)
    mp = host.model_prob(1, 0.2, base_freq=BF)
    for name, halves, seed in (("R64", (8, 30), 31), ("R40", (40, 70), 32), ("R256", (100, 140), 33)):
        band = random_tunnel(np.random.default_rng(seed), gl.n_sites - 1, gr.n_sites - 1, *halves)
        p = fx.Pair(name, gl, gr, mp, band, host.dna_model(BF, 0.2)[0])
        _lf, _lb, opost, _ologf = oracle.fb(gl, gr, mp, band=band)
        out[name] = Case(p, pycheck_mea.exact_arcs(gl, gr, mp, band), opost)
    # asymmetric tables, tables with zeros, 211 and 1892 states, 512 and 1,024 threads (fb_tables.py): the leaf pairs on the
    # oracle's posterior, the 71 x 67 graph pairs on the exact reading's
    leaves = fb_tables.leaf_pairs()
    fb_tables.check_shapes(leaves)
    leaves["K1892"] = fb_tables.codon_leaf_pair(oracle)
    # the root jobs of a four-leaf protein and a four-leaf codon walk: graph against graph, ancestral states (>= 20, > 61)
    leaves["G211w"], leaves["K1892g"] = fb_tables.walk_root_pair(2), fb_tables.walk_root_pair(3, oracle)
    for name, p in leaves.items():
        lf, _lb, opost, _ologf = oracle.fb(p.left, p.right, p.mp, band=p.band)
        assert np.isfinite(lf), name
        out[name] = Case(p, pycheck_mea.exact_arcs(p.left, p.right, p.mp, p.band), opost)
    for name, p in fb_tables.graph_pairs().items():
        ex = pycheck_fb.Exact(*p.args())
        assert np.isfinite(ex.log_fwd), name
        out[name] = Case(p, ex, ex.posterior())
    for name, c in out.items():
        if getattr(c.p, "before", None) is not None:             # the zeros decide the result (fb_tables.zeros_bite)
            counts = fb_tables.zeros_bite(c.p, pycheck_mea.exact_arcs(c.p.left, c.p.right, c.p.before, c.p.band), c.mea(0.5))
            print("%s: zero entries that a skipped / transposed (-inf, finite) lookup shows, transposed zeros on the path: %s" % (name, counts))
    return out


# pair -> (threads of the decode's workgroup, the instance looks the table up (TAB), the table is in LDS): what
# pagan_fb_decode_batch must launch, asserted against the host-only plan and the table
INSTANCES = {"R257": (512, False, True), "R512z": (512, True, True), "R513": (1024, False, True), "R513z": (1024, True, True),
             "Q64z": (64, True, False), "Q257z": (512, True, False), "Q513z": (1024, True, False), "K1892": (64, False, False)}


def check_instance(name, p, fb):
    """the instance from what the library reports: the launch's threads and lookup flag (pagan_fb_decoded_launch), the plan's
    decode_block and table_in_lds"""
    block, tab, lds = INSTANCES[name]
    mw, _nd = widest_diagonal(p)
    plan = pgm.fb_plan(p.left, p.right, p.band, p.mp.n_states)
    dec = fb.decode(0.5)
    threads, looked = dec.launch()
    dec.close()
    assert threads == plan["decode_block"] and tab == bool((p.mp.score == 0).any())
    got = (threads, looked, bool(plan["table_in_lds"]))
    print("%s: widest diagonal %d, pg_fb_ring_decode<%d, %s> with %d threads, table in %s"
          % (name, mw, 1024 if got[0] > 512 else 512, "true" if got[1] else "false", got[0], "LDS" if got[2] else "memory"))
    assert plan["decode_route"] == 1 and got == (block, tab, lds) and block == fb_tables.block_for(mw), (name, got, mw)


def check_decode(case, g, fb, schedule, what):
    """everything a case asserts; returns (DecodedPath summary, visited, device matrix)"""
    p, ex = case.p, case.ex
    ref = case.mea(g)
    dec = fb.decode(g, keep_matrix=True)
    sm = dec.summary()
    print("%s g %.1f: schedule %d status %d objective %.12g (reference %.12g) steps %d" %
          (what, g, sm["schedule"], sm["status"], sm["objective"], ref.objective, sm["n_steps"]))
    assert sm["schedule"] == schedule and sm["status"] == ref.status, (what, sm)
    A = dec.matrix()
    fin = np.isfinite(ref.A)
    assert not np.isnan(A).any() and np.array_equal(np.isfinite(A), fin) and np.all(np.isneginf(A[~fin])), what
    ij = (np.arange(p.Lx)[:, None, None] + np.arange(p.Ly)[None, :, None] + 1) * np.ones((1, 1, 3))
    err = np.abs(A[fin] - ref.A[fin])
    print("   largest |A_dev - A_ref| %.3g over %d finite cells" % (err.max() if err.size else 0.0, int(fin.sum())))
    assert np.all(err <= bound(ref.A[fin], ij[fin])), (what, err.max())
    vis = dec.visited()
    assert sm["n_steps"] == vis.shape[0]
    assert [sm["n_x"], sm["n_y"], sm["n_m"]] == [int((vis[:, 2] == s).sum()) for s in (0, 1, 2)], what
    res = dec.result()
    if ref.status == 1:
        assert sm["objective"] == 0.0 and sm["n_steps"] == 0 and fb.log_fwd == -np.inf, what
        assert res.status == abi.PAGAN_DP_UNREACHABLE and res.cols.shape[0] == 0
        dec.close()
        return sm, vis, A
    tol = bound(ref.objective, vis.shape[0] + 1)
    assert abs(sm["objective"] - ref.objective) <= tol, (what, sm["objective"], ref.objective)
    assert res.status == 0 and res.score == fb.log_fwd, what
    assert pycheck_mea.is_path(ex, vis, res.end[:3]), what
    on_ref = pycheck_mea.objective_of(ref.w, vis)
    assert on_ref >= ref.objective - tol, (what, on_ref, ref.objective)
    # the replay's columns sit on the visited cells, start -> end
    cells = pgm.path_cells(res.cols)
    cells = cells[cells[:, 0] >= 0]
    assert np.array_equal(cells[:, [1, 2, 0]], vis[::-1]), what
    dec.close()
    return sm, vis, A


# (pair, sweep environment, sweep schedule, decode ring switch, decode schedule, gap weights)
CASES = [
    ("P1", "default", 0, None, 0, (0.5,)),
    ("P1t", "default", 0, None, 0, (0.5, 0.0, 1.0)), ("P1t", "band", 1, None, 0, (0.5,)), ("P1t", "deep", 3, None, 0, (0.5,)),
    ("P2", "default", 0, None, 0, (0.5,)), ("P2t", "default", 0, None, 0, (0.5,)),
    ("P3t", "default", 0, None, 0, (0.5,)),
    ("P4at", "default", 0, None, 0, (0.5,)), ("P4bt", "default", 0, None, 0, (0.5,)),
    ("P5t", "ring", 2, None, 1, (0.5, 0.0, 1.0)), ("P5t", "default", 0, None, 1, (0.5,)), ("P5t", "ring", 2, "0", 0, (0.5, 0.0, 1.0)),
    ("P5z", "default", 0, None, 1, (0.5,)), ("P5z", "default", 0, "0", 0, (0.5,)),
    ("P6a", "default", 0, None, 0, (0.5,)), ("P6b", "default", 0, None, 0, (0.5,)),
    ("R64", "default", 2, None, 1, (0.5,)), ("R64", "default", 2, "0", 0, (0.5,)),
    ("R40", "default", 2, None, 1, (0.5,)), ("R256", "default", 2, None, 1, (0.5,)),
    ("R257", "default", 2, None, 1, (0.5,)), ("R512z", "default", 2, None, 1, (0.5,)),
    ("R513", "default", 2, None, 1, (0.5,)), ("R513z", "default", 2, None, 1, (0.5,)), ("R513z", "default", 2, "0", 0, (0.5,)),
    ("Q64z", "default", 2, None, 1, (0.5,)), ("Q64z", "default", 2, "0", 0, (0.5,)),
    ("Q257z", "default", 2, None, 1, (0.5,)), ("Q513z", "default", 2, None, 1, (0.5,)),
    ("G211", "default", 0, None, 0, (0.5,)), ("G211z", "default", 0, None, 0, (0.5, 0.0, 1.0)),
    ("K1892", "default", 0, None, 1, (0.5,)),
    ("G211w", "default", 0, None, 0, (0.5,)), ("K1892g", "default", 0, None, 0, (0.5,)),
]


@pytest.mark.parametrize("name, env, sweep, ring, schedule, gs", CASES, ids=["%s-%s-%s-%d" % (c[0], c[1], c[3], c[4]) for c in CASES])
def test_decode_against_the_second_reading(pg, cases, monkeypatch, name, env, sweep, ring, schedule, gs):
    fx.set_env(monkeypatch, env)
    monkeypatch.delenv(DECODE_ENV, raising=False)
    if ring is not None:
        monkeypatch.setenv(DECODE_ENV, ring)
    case = cases[name]
    p = case.p
    assert pgm.fb_decode_route(p.left, p.right, p.band) == schedule
    if name == "R64":
        mw, nd = widest_diagonal(p)
        assert mw <= 64 and nd > 512, (mw, nd)
    if name == "R40":
        mw, nd = widest_diagonal(p)
        assert 32 < mw <= 64 and nd > 512, (mw, nd)
    if name == "R256":
        mw, nd = widest_diagonal(p)
        assert 128 < mw <= 256 and nd > 512, (mw, nd)
    if name == "P3t":
        assert case.mea(0.5).status == 1
    if name.startswith("G211"):
        assert p.mp.n_states == 211 and case.mea(0.5).status == 0
    fb = pgm.FullProbability(*p.args())
    assert fb.schedule == sweep, (name, env, fb.schedule)
    if name in INSTANCES and ring is None:
        check_instance(name, p, fb)
    assert np.allclose(fb.posterior(), case.post, rtol=1e-7, atol=1e-12)       # (what the bound rests on)
    for g in gs:
        check_decode(case, g, fb, schedule, "%s after the %s sweeps" % (name, env))
    fb.close()


def test_ring_and_fill_agree(pg, cases, monkeypatch):
    """P5t, the 300 x 290 pair, and the zero tables from memory and on 1,024 threads, on both routes: equal -inf sets,
    objectives within the bound of one another."""
    for name in ("P5t", "R64", "Q64z", "R513z"):
        p = cases[name].p
        fx.set_env(monkeypatch, "default")
        fb = pgm.FullProbability(*p.args())
        monkeypatch.delenv(DECODE_ENV, raising=False)
        ring = fb.decode(0.5, keep_matrix=True)
        monkeypatch.setenv(DECODE_ENV, "0")
        fill = fb.decode(0.5, keep_matrix=True)
        a, b = ring.summary(), fill.summary()
        assert (a["schedule"], b["schedule"]) == (1, 0) and a["status"] == b["status"] == 0
        assert abs(a["objective"] - b["objective"]) <= bound(b["objective"], b["n_steps"] + 1)
        A, B = ring.matrix(), fill.matrix()
        assert np.array_equal(np.isfinite(A), np.isfinite(B))
        fin = np.isfinite(B)
        assert np.all(np.abs(A[fin] - B[fin]) <= bound(B[fin], p.Lx + p.Ly))
        for d in (ring, fill):
            d.close()
        fb.close()


def test_the_1024_thread_windows_on_a_full_workgroup(pg, monkeypatch):
    """R1024z: 1,024 x 1,300 cells under the DNA zero table -- every thread of pg_fb_ring_decode<1024, true> has a row, and the
    row and column windows' live span (the diagonal's width + FB_RG_REFILL + 1 entries at a refill) passes 1,024 entries, which
    no pair narrower than 769 cells, nor any whose longer side stays below 1,024 + the window's first column, can show
    (fb_tables.stale_window_cells counts the cells a 1,024-entry window would serve a wrong state: test_mea_cpu.py).  No second
    reading of 1.3 M cells: the ring against the PAGAN_FB_DECODE_RING=0 fill, which reads no window and whose lookup the 71 x 67
    and 513-wide cases hold to the reading, within the bound; and the match scores finite exactly where the table's entry is
    above 0 -- in a full matrix every cell is reached through gaps, so the lookup alone decides."""
    p = fb_tables.wide_zero_pair()
    assert (p.Lx, p.Ly) == (1024, 1300) and widest_diagonal(p)[0] == 1024
    fx.set_env(monkeypatch, "default")
    fb = pgm.FullProbability(*p.args())
    monkeypatch.delenv(DECODE_ENV, raising=False)
    ring = fb.decode(0.5, keep_matrix=True)
    monkeypatch.setenv(DECODE_ENV, "0")
    fill = fb.decode(0.5, keep_matrix=True)
    a, b = ring.summary(), fill.summary()
    assert (a["schedule"], b["schedule"]) == (1, 0) and a["status"] == b["status"] == 0 and ring.launch() == (1024, True)
    assert abs(a["objective"] - b["objective"]) <= bound(b["objective"], b["n_steps"] + 1)
    A, B = ring.matrix(), fill.matrix()
    entry = fb_tables.entries(p)
    for name, mat in (("ring", A), ("fill", B)):
        assert np.array_equal(np.isfinite(mat[1:, 1:, 2]), entry[1:, 1:] > 0), name
        assert np.isfinite(mat[1:, :, 0]).all() and np.isfinite(mat[:, 1:, 1]).all(), name
    fin = np.isfinite(B)
    assert np.array_equal(np.isfinite(A), fin)
    assert np.all(np.abs(A[fin] - B[fin]) <= bound(B[fin], p.Lx + p.Ly))
    for d in (ring, fill):
        d.close()
    fb.close()


def _bytes(d):
    sm = d.summary()
    return repr(sorted(sm.items())).encode() + d.visited().tobytes() + d.matrix().tobytes()


def test_batch_equals_single(pg, cases, monkeypatch):
    """One call over ring pairs of two workgroup sizes, fill pairs and a pair of total 0: the single calls' summaries, traces and
    kept matrices, byte for byte; the launches' times are booked at the first pair."""
    fx.set_env(monkeypatch, "default")
    monkeypatch.delenv(DECODE_ENV, raising=False)
    names = ["P1t", "P5t", "P3t", "R256", "P5z", "R64", "P4bt"]
    fbs = [pgm.FullProbability(*cases[n].p.args()) for n in names]
    batch = pgm.decode_batch(fbs, 0.5, keep_matrix=True)
    assert [b.summary()["schedule"] for b in batch] == [0, 1, 0, 1, 1, 1, 0]
    assert [b.summary()["status"] for b in batch] == [0, 0, 1, 0, 0, 0, 0]
    ms = [b.ms() for b in batch]
    assert ms[0][0] > 0 and ms[0][1] > 0 and all(m == (0.0, 0.0) for m in ms[1:])
    for n, fb, b in zip(names, fbs, batch):
        single = fb.decode(0.5, keep_matrix=True)
        assert _bytes(single) == _bytes(b), n
        single.close()
    # a decoded handle outlives its pair
    want = _bytes(batch[1])
    for fb in fbs:
        fb.close()
    assert _bytes(batch[1]) == want and batch[1].result().status == 0
    for b in batch:
        b.close()
    # the fill and five ring launch keys -- <512, false> at 64 and at 512 threads, <512, true> at 64, <1024, false>, <1024, true>
    # twice --; the call's order has the pair with the lookup behind the one without at 1,024 threads and in front of it at 64
    names = ["R513", "Q64z", "R513z", "P1t", "R257", "Q513z", "K1892"]
    fbs = [pgm.FullProbability(*cases[n].p.args()) for n in names]
    batch = pgm.decode_batch(fbs, 0.5, keep_matrix=True)
    assert [b.summary()["schedule"] for b in batch] == [1, 1, 1, 0, 1, 1, 1]
    assert all(b.summary()["status"] == 0 for b in batch)
    for n, fb, b in zip(names, fbs, batch):
        single = fb.decode(0.5, keep_matrix=True)
        assert _bytes(single) == _bytes(b), n
        single.close()
    for x in batch + fbs:
        x.close()


def test_arguments(pg, cases):
    p = cases["P6b"].p
    fb = pgm.FullProbability(*p.args())
    for bad in (-0.5, float("nan"), float("inf")):
        with pytest.raises(pgm.PaganError) as e:
            fb.decode(bad)
        assert e.value.code == abi.PAGAN_E_ARG
    L = pgm.lib()
    out = (C.c_void_p * 2)()
    assert L.pagan_fb_decode(None, 0.5, 0, out) == abi.PAGAN_E_ARG
    handles = (C.c_void_p * 2)(fb._h, None)
    assert L.pagan_fb_decode_batch(2, handles, 0.5, 0, out) == abi.PAGAN_E_ARG
    assert L.pagan_fb_decode(fb._h, 0.5, 2, out) == abi.PAGAN_E_ARG                  # an unknown flag
    assert not out[0] and not out[1]
    dec = fb.decode()
    assert dec.summary()["status"] == 0
    with pytest.raises(pgm.PaganError) as e:
        dec.matrix()
    assert e.value.code == abi.PAGAN_E_ARG
    dec.close()
    fb.close()


def _sum_on(w, cells):
    """cells: rows (state, i, j), -1 at skip columns (pagan_path_cells)"""
    c = cells[cells[:, 0] >= 0]
    return float(w[c[:, 1], c[:, 2], c[:, 0]].sum())


@pytest.mark.parametrize("name", ["P1t", "R64"])
def test_no_path_that_exists_beats_the_decoded_one(pg, cases, monkeypatch, name):
    """On the device's own weights: the Viterbi path (align with the log-space model) and 64 sampled paths are paths of the set
    the decode maximises over."""
    fx.set_env(monkeypatch, "default")
    monkeypatch.delenv(DECODE_ENV, raising=False)
    p = cases[name].p
    fb = pgm.FullProbability(*p.args())
    w = pycheck_mea.weights(fb.posterior(), 0.5)
    dec = fb.decode(0.5)
    sm = dec.summary()
    vis = dec.visited()
    own = pycheck_mea.objective_of(w, vis)
    tol = bound(own, vis.shape[0] + 1)
    assert abs(own - sm["objective"]) <= tol
    vit = pgm.align(p.left, p.right, p.model, p.band)
    assert vit.status == 0
    v_obj = _sum_on(w, pgm.path_cells(vit.cols))
    sp = fb.sample_paths(7, 1, 64)
    assert np.all(sp.summary()["status"] == 0)
    allv, alln = sp.visited_all()
    s_obj = [pycheck_mea.objective_of(w, allv[q, :alln[q]]) for q in range(64)]
    print("%s: decoded %.6f, Viterbi %.6f, sampled %.6f .. %.6f" % (name, own, v_obj, min(s_obj), max(s_obj)))
    assert own >= v_obj - tol and own >= max(s_obj) - tol
    sp.close()
    dec.close()
    fb.close()


def test_the_walk_decodes_every_node(pg):
    names, seqs, nwk = synth.evolve_balanced(8, 120, branch=0.05, sub=0.05, indel_start=0.02, mean_len=3, seed=53)
    opts = {"use_anchors": 1, "prefix_hit_length": 8}
    walk = host.Msa(names, seqs, nwk, posterior_decode=1, decode_gap_weight=0.5, **opts).align()
    by_node = host.Msa(names, seqs, nwk, posterior_decode=1, decode_gap_weight=0.5, **opts)
    while by_node.remaining > 0:
        by_node.align_nodes(by_node.ready()[-1:])
    by_node.finish()
    assert walk.alignment_all() == by_node.alignment_all()
    for row, seq in zip(walk.alignment(), seqs):
        assert row.replace("-", "") == seq
    schedules = set()
    booked = 0
    for k in range(walk.n_internal):
        left, right, _model, band = walk.node_job(k)
        fb = pgm.FullProbability(left, right, walk.node_model_prob(k), band)
        dec = fb.decode(0.5)
        want, sm = dec.result(), dec.summary()
        schedules.add(sm["schedule"])
        for w in (walk, by_node):
            got = w.node_result(k)
            assert got.status == 0 and np.array_equal(got.cols, want.cols), k
            assert np.array_equal(got.left_used, want.left_used) and np.array_equal(got.right_used, want.right_used), k
            obj, steps, ms = w.node_decode(k)
            assert obj == sm["objective"] and steps == sm["n_steps"] and ms >= 0, k
            assert w.node_info(k).score == fb.log_fwd == w.node_fb(k)[0]
            assert w.node_support(k).tobytes() == fb.path_support(want.cols).tobytes(), k
        booked += walk.node_decode(k)[2] > 0
        dec.close()
        fb.close()
    assert schedules == {0, 1} and booked >= 1          # (leaf pairs on the ring, graph pairs on the fill)
    off = host.Msa(names, seqs, nwk, **opts).align()
    with pytest.raises(pgm.PaganError) as e:
        off.node_decode(0)
    assert e.value.code == abi.PAGAN_E_ARG
    both = host.Msa(names, seqs, nwk, posterior_decode=1, sample_path=1, **opts)
    with pytest.raises(pgm.PaganError) as e:
        both.align()
    assert e.value.code == abi.PAGAN_E_ARG


@pytest.mark.parametrize("data_type", [2, 3])
def test_the_walk_decodes_every_node_under_the_large_tables(pg, data_type):
    """Four protein leaves of ~60 residues, four codon leaves of ~40 codons, posterior_decode=1: every node is the stand-alone
    FullProbability -> decode chain on node_job(k) and node_model_prob(k) (211 and 1892 states: the table read from memory by
    the ring at the leaves, by the fill and the trace above them), as test_the_walk_decodes_every_node has it for DNA."""
    if data_type == 2:
        names, seqs, nwk = synth.evolve_balanced(4, 60, branch=0.08, sub=0.1, indel_start=0.03, mean_len=3, seed=57, alphabet=fb_tables.AA)
    else:
        names, seqs, nwk = fb_tables.evolve_codons(4, 40, seed=58, branch=0.08, sub=0.1, indel_start=0.03, mean_len=2)
    walk = host.Msa(names, seqs, nwk, posterior_decode=1, decode_gap_weight=0.5, data_type=data_type, use_anchors=0).align()
    assert walk.n_internal == 3 and walk.data_type == data_type
    schedules, top = set(), 0
    for k in range(walk.n_internal):
        left, right, _model, band = walk.node_job(k)
        mp = walk.node_model_prob(k)
        assert mp.n_states == (211 if data_type == 2 else 1892)
        top = max(top, int(left.state[1:-1].max()), int(right.state[1:-1].max()))
        fb = pgm.FullProbability(left, right, mp, band)
        dec = fb.decode(0.5)
        want, sm = dec.result(), dec.summary()
        schedules.add(sm["schedule"])
        got = walk.node_result(k)
        assert sm["status"] == 0 and got.status == 0 and np.array_equal(got.cols, want.cols), k
        assert np.array_equal(got.left_used, want.left_used) and np.array_equal(got.right_used, want.right_used), k
        obj, steps, ms = walk.node_decode(k)
        assert obj == sm["objective"] and steps == sm["n_steps"] and ms >= 0, k
        assert walk.node_info(k).score == fb.log_fwd == walk.node_fb(k)[0]
        assert walk.node_support(k).tobytes() == fb.path_support(want.cols).tobytes(), k
        dec.close()
        fb.close()
    assert schedules == {0, 1}                                   # (the leaf pairs on the ring, the root on the fill)
    assert top >= (20 if data_type == 2 else 62)                 # (an ancestral state entered the root's pair)
