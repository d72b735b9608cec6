"""GPU: the deep-ring forward/backward sweeps for graph pairs inside tunnels (dp_fb_deep.inc: pg_fb_forward_deep /
pg_fb_backward_deep; schedule code 3) against the oracle's log-space restatement (oracle/oracle_fb.cpp), at the tolerances of
test_fb_gpu.py: 1e-9 on logs, 1e-7 relative on posteriors.  No case may take another schedule: a pair that does not come out as
schedule 3 is a failure."""
import numpy as np
import pytest

import pagan2_msa_amd as pgm
from pagan2_msa_amd import abi, host, synth

pytestmark = pytest.mark.gpu
LOG_TOL = 1e-9

# (leaves, length, seed) of the DNA trees; every internal node above the leaves is a case, behind one random tunnel of each range of
# half-widths.  Fixed on the CPU with fb_route (tests/diagnostics/sweep_fb_deep.py --route-only walks the same trees with the oracle):
# under PAGAN_FB_DEEP_MIN_ND=0 all of them route to schedule 3.
TREES = [(4, 700, 46), (8, 700, 46), (16, 400, 52)]
HALVES = ((5, 12), (20, 70), (100, 180))       # the half-widths of test_ring_sweeps_cell_by_cell: widest diagonals of ~11, ~55, ~150 cells (B = 64, 64, 256)
HALF_128 = (70, 125)                           # ... and one more range for the widths between 64 and 128 cells (B = 128, D = 32)


def close_logs(a, b):
    fa, fb = np.isfinite(a), np.isfinite(b)
    return np.array_equal(fa, fb) and np.allclose(a[fa], b[fb], rtol=LOG_TOL, atol=LOG_TOL)


def _random_tunnel(rng, Lx, Ly, lo_half, hi_half):
    half = rng.integers(lo_half, hi_half, Lx)
    centre = np.arange(Lx) * (Ly - 1) // max(Lx - 1, 1)
    upper = np.maximum.accumulate(np.maximum(centre - half, 0))
    lower = np.maximum.accumulate(np.minimum(centre + half, Ly - 1))
    upper[0] = 0
    lower[-1] = Ly - 1
    return abi.Band(upper.astype(np.int32), lower.astype(np.int32))


def _boxed_tunnel(Lx, Ly, boxes, half=8):
    """a narrow band around the main diagonal with square boxes [(first row, side), ...] that hold every cell of their rows x columns"""
    centre = np.arange(Lx) * (Ly - 1) // max(Lx - 1, 1)
    upper, lower = np.maximum(centre - half, 0), np.minimum(centre + half, Ly - 1)
    for a, w in boxes:
        upper[a:a + w] = np.minimum(upper[a:a + w], max(centre[a] - half, 0))
        lower[a:a + w] = np.maximum(lower[a:a + w], min(centre[a + w - 1] + half, Ly - 1))
    upper, lower = np.maximum.accumulate(upper), np.maximum.accumulate(lower)
    upper[0] = 0
    lower[-1] = Ly - 1
    return abi.Band(upper.astype(np.int32), lower.astype(np.int32))


def multi_edge_sites(g):
    return int((np.diff(g.bwd_off) > 1).sum())


def is_plain(g):
    n = g.n_sites
    return bool(np.all(np.diff(g.bwd_off)[1:] == 1) and np.array_equal(g.bwd_src[:n - 1], np.arange(n - 1)))


def upper_pairs(names, seqs, nwk, data_type=1, **opts):
    """[(left, right, model_prob)] of every internal node above the leaves (at least one child is a graph)"""
    if data_type != 1:
        opts = dict(opts, data_type=data_type)
    msa = host.Msa(names, seqs, nwk, **opts).align()
    if data_type == 1:
        bf = np.array([sum(s.count(x) for s in seqs) for x in "ACGT"], np.float32)
        bf /= bf.sum()
    out = []
    for k in range(msa.n_internal):
        left, right, _model, _band = msa.node_job(k)
        if is_plain(left) and is_plain(right):
            continue
        mp = host.model_prob(1, msa.node_info(k).dist, base_freq=bf) if data_type == 1 else host.model_prob(data_type, msa.node_info(k).dist)
        out.append((left, right, mp))
    return out


def far_meets_multi(g, D):
    """sites with more than one edge of which one reaches D or further back"""
    off = g.bwd_off.astype(np.int64)
    n = 0
    for i in range(1, g.n_sites - 1):
        if off[i + 1] - off[i] > 1 and int(i - g.bwd_src[off[i]:off[i + 1]].min()) >= D:
            n += 1
    return n


def check_deep(oracle, left, right, mp, band):
    code, info = pgm.fb_route(left, right, band)
    assert code == 3, (code, info)
    fb = pgm.FullProbability(left, right, mp, band)
    assert fb.schedule == 3 and fb.groups == 0, (fb.schedule, info)
    lf, lb, post, logf = oracle.fb(left, right, mp, band=band)
    print("deep pair %d x %d: %s | log_fwd %.12g (oracle %.12g) log_bwd %.12g (oracle %.12g)" % (left.n_sites - 1, right.n_sites - 1, info, fb.log_fwd, lf, fb.log_bwd, lb))
    assert abs(fb.log_fwd - lf) <= LOG_TOL * max(1, abs(lf)), (fb.log_fwd, lf, info)
    assert abs(fb.log_bwd - lb) <= LOG_TOL * max(1, abs(lb)), (fb.log_bwd, lb, info)
    assert abs(fb.log_fwd - fb.log_bwd) <= 1e-7 * abs(fb.log_fwd)
    assert close_logs(fb.log_forward(), logf), info
    assert np.allclose(fb.posterior(), post, rtol=1e-7, atol=1e-12), info
    return fb, info, logf


def test_graph_pairs_behind_random_tunnels_cell_by_cell(pg, oracle, monkeypatch):
    """Every internal node above the leaves of trees of 4, 8 and 16 leaves, behind random tunnels of three ranges of half-widths
    (B = 64 ... 256, hence D = 64 ... 16): every cell of the forward matrix and every posterior against the oracle."""
    monkeypatch.setenv("PAGAN_FB_DEEP_MIN_ND", "0")
    rng = np.random.default_rng(2027)
    multi, far_cells, far_multi, min_ds, n = 0, 0, 0, set(), 0
    for leaves, length, seed in TREES:
        names, seqs, nwk = synth.evolve_balanced(leaves, length, branch=0.04, sub=0.04, indel_start=0.01, mean_len=4, seed=seed)
        for q, (left, right, mp) in enumerate(upper_pairs(names, seqs, nwk, use_anchors=0)):
            for lo_half, hi_half in (HALVES + (HALF_128,) if leaves < 16 else (HALVES[q % 3],)):
                band = _random_tunnel(rng, left.n_sites - 1, right.n_sites - 1, lo_half, hi_half)
                fb, info, _ = check_deep(oracle, left, right, mp, band)
                fb.close()
                multi += multi_edge_sites(left) + multi_edge_sites(right)
                far_cells += info["far_cells"]
                if info["far_cells"] > 0:
                    far_multi += far_meets_multi(left, info["min_D"]) + far_meets_multi(right, info["min_D"])
                min_ds.add(info["min_D"])
                n += 1
    assert n >= 4 + 3 * 4 + 7 and multi > 0
    assert {16, 32, 64} <= min_ds, min_ds                  # B = 256, 128, 64 all reached
    assert far_cells > 0 and far_multi > 0                 # edges that reach past a ring of 16 diagonals, some of them at multi-edge sites


def test_protein_tree_table_in_memory(pg, oracle, monkeypatch):
    """211 states: the score table does not fit LDS (the kernels' other instantiation)."""
    monkeypatch.setenv("PAGAN_FB_DEEP_MIN_ND", "0")
    aa = "ARNDCQEGHILKMFPSTWYV"
    names, seqs, nwk = synth.evolve_balanced(4, 300, branch=0.05, sub=0.08, indel_start=0.012, mean_len=3, seed=42, alphabet=aa)
    pairs = upper_pairs(names, seqs, nwk, data_type=2, use_anchors=0)
    assert pairs
    rng = np.random.default_rng(9)
    for left, right, mp in pairs:
        assert multi_edge_sites(left) + multi_edge_sites(right) > 0
        fb, _info, _ = check_deep(oracle, left, right, mp, _random_tunnel(rng, left.n_sites - 1, right.n_sites - 1, 20, 70))
        fb.close()


def test_boxed_tunnel_changes_the_ring_shape_inside_one_pair(pg, oracle, monkeypatch):
    """A narrow band with two boxes of ~400 and ~900 columns: segments of B = 64, 512 and 1,024 in one pair, a boundary in each
    direction; inside the B = 1,024 segment every edge of reach >= 4 is far, and multi-edge sites have such edges."""
    monkeypatch.setenv("PAGAN_FB_DEEP_MIN_ND", "0")
    names, seqs, nwk = synth.evolve_balanced(4, 2600, branch=0.04, sub=0.04, indel_start=0.01, mean_len=4, seed=48)
    left, right, mp = upper_pairs(names, seqs, nwk, use_anchors=0)[-1]
    Lx, Ly = left.n_sites - 1, right.n_sites - 1
    band = _boxed_tunnel(Lx, Ly, [(300, 400), (1200, 900)])
    fb, info, _ = check_deep(oracle, left, right, mp, band)
    fb.close()
    assert info["segments"] > 1 and info["min_D"] == 4, info
    assert 512 < info["widest"] <= 1024, info
    assert info["far_cells"] > 0 and 0 < info["far_diagonals"] < info["diagonals"], info
    assert far_meets_multi(left, 4) + far_meets_multi(right, 4) > 0


def test_long_pair_by_default_and_sampling(pg, oracle, monkeypatch):
    """The root pair of 4 x 2.5 kb inside its define_tunnel band (5,000 cell diagonals, beyond the default threshold) with the
    default environment: schedule 3, totals against the oracle; paths sampled from its forward matrix against the oracle's."""
    for v in ("PAGAN_FB_DEEP", "PAGAN_FB_DEEP_MIN_ND", "PAGAN_FB_BAND_MIN_ND", "PAGAN_FB_RING_MIN_ND", "PAGAN_FB_GROUPS"):
        monkeypatch.delenv(v, raising=False)
    names, seqs, nwk = synth.evolve_balanced(4, 2500, branch=0.01, sub=0.01, indel_start=0.008, mean_len=4, seed=61)
    msa = host.Msa(names, seqs, nwk, use_anchors=1).align()
    k = msa.n_internal - 1
    left, right, _model, band = msa.node_job(k)
    bf = np.array([sum(s.count(x) for s in seqs) for x in "ACGT"], np.float32)
    bf /= bf.sum()
    mp = host.model_prob(1, msa.node_info(k).dist, base_freq=bf)
    code, info = pgm.fb_route(left, right, band)
    assert code == 3 and info["diagonals"] >= 4096, (code, info)
    fb = pgm.FullProbability(left, right, mp, band)
    assert fb.schedule == 3
    lf, lb, _, logf = oracle.fb(left, right, mp, band=band)
    assert abs(fb.log_fwd - lf) <= LOG_TOL * max(1, abs(lf)) and abs(fb.log_bwd - lb) <= LOG_TOL * max(1, abs(lb)), (fb.log_fwd, lf, fb.log_bwd, lb)
    assert abs(fb.log_fwd - fb.log_bwd) <= 1e-7 * abs(fb.log_fwd)
    rng = np.random.default_rng(6)
    for _ in range(3):
        u = rng.random(left.n_sites + right.n_sites)
        res, visited = fb.sample_path(u)
        want, _end = oracle.sample_path(left, right, mp, logf, u)
        assert np.array_equal(visited, want)
        assert res.status == 0 and res.score == fb.log_fwd
        assert [c for c in res.cols[:, 0] if c >= 0] == list(range(1, left.n_sites - 1))
        assert [c for c in res.cols[:, 1] if c >= 0] == list(range(1, right.n_sites - 1))
    fb.close()
    # the switch gives the pair back to the block schedule, with the same sums
    monkeypatch.setenv("PAGAN_FB_DEEP", "0")
    fb0 = pgm.FullProbability(left, right, mp, band)
    assert fb0.schedule == 1 and fb0.groups > 1
    assert abs(fb0.log_fwd - lf) <= LOG_TOL * max(1, abs(lf)) and abs(fb0.log_bwd - lb) <= LOG_TOL * max(1, abs(lb))
    fb0.close()


def _mixed_cases(monkeypatch, reps, per_rep=None):
    """(cases, n_deep, the schedules they route to): deep-ring pairs of the 8-leaf tree behind a random tunnel per `reps` entry (the
    range of half-widths HALVES[rep % 3], `per_rep` pairs each: all), then a plain-ring pair, two tiled pairs and a small one --
    all of at most 700 sites"""
    for v in ("PAGAN_FB_DEEP", "PAGAN_FB_BAND_MIN_ND", "PAGAN_FB_RING_MIN_ND", "PAGAN_FB_GROUPS"):
        monkeypatch.delenv(v, raising=False)
    monkeypatch.setenv("PAGAN_FB_DEEP_MIN_ND", "1000")
    rng = np.random.default_rng(31)
    names, seqs, nwk = synth.evolve_balanced(8, 700, branch=0.04, sub=0.04, indel_start=0.01, mean_len=4, seed=46)
    ups = upper_pairs(names, seqs, nwk, use_anchors=0)
    cases = []
    for rep in reps:
        for left, right, mp in ups[:per_rep]:
            lo_half, hi_half = HALVES[rep % 3]
            cases.append((left, right, mp, _random_tunnel(rng, left.n_sites - 1, right.n_sites - 1, lo_half, hi_half)))     # deep ring
    n_deep = len(cases)
    gl, gr = (host.HGraph.leaf(s).flatten() for s in seqs[:2])
    mpl = host.model_prob(1, 0.08, base_freq=[0.25] * 4)
    cases.append((gl, gr, mpl, _random_tunnel(rng, gl.n_sites - 1, gr.n_sites - 1, 20, 70)))       # plain ring
    cases.append((ups[0][0], ups[0][1], ups[0][2], None))                                         # graph pairs without a band: tiled
    cases.append((ups[2][0], ups[2][1], ups[2][2], None))
    _, short, _ = synth.evolve_balanced(2, 100, branch=0.05, sub=0.05, indel_start=0.01, mean_len=3, seed=3)
    sl, sr = (host.HGraph.leaf(s).flatten() for s in short)
    cases.append((sl, sr, mpl, None))                                                             # small: one-workgroup kernels
    want_sched = [3] * n_deep + [2, 1, 1, 0]
    assert [pgm.fb_route(c[0], c[1], c[3])[0] for c in cases] == want_sched
    return cases, n_deep, want_sched


def _second_size(cases, n_deep):
    """the first deep pair whose workgroup size is not the first deep pair's (widest diagonal beyond 64 cells or not)"""
    wide = [pgm.fb_route(c[0], c[1], c[3])[1]["widest"] > 64 for c in cases[:n_deep]]
    assert len(set(wide)) == 2                                                                    # two workgroup sizes among the deep pairs
    return wide.index(not wide[0])


def test_a_batch_mixes_deep_ring_pairs_with_the_other_schedules(pg, oracle, monkeypatch):
    """full_probability_batch on deep-ring pairs (18, of two workgroup sizes), plain-ring, tiled and small pairs: every handle's
    totals bit-equal to the one-pair call's, schedules as routed.  The one-pair call is the batch of one, so the oracle anchors
    the batch itself: one pair of each schedule, and a deep pair of the second workgroup size, to LOG_TOL."""
    cases, n_deep, want_sched = _mixed_cases(monkeypatch, range(6))
    assert n_deep >= 16
    second = _second_size(cases, n_deep)
    single = []
    for c in cases:
        fb = pgm.FullProbability(*c)
        single.append((fb.log_fwd, fb.log_bwd, fb.schedule))
        fb.close()
    assert [s[2] for s in single] == want_sched
    fbs = pgm.full_probability_batch(cases)
    assert [fb.schedule for fb in fbs] == [pgm.fb_route(c[0], c[1], c[3])[0] for c in cases]     # the plan's code, same environment
    for k in (0, second, n_deep, n_deep + 1, n_deep + 3):                  # deep, deep of the other size, ring, tiled, small
        lf, lb, _, _ = oracle.fb(*cases[k][:3], band=cases[k][3], matrices=False)
        print("pair %d (schedule %d): log_fwd %.12g (oracle %.12g) log_bwd %.12g (oracle %.12g)" % (k, fbs[k].schedule, fbs[k].log_fwd, lf, fbs[k].log_bwd, lb))
        assert abs(fbs[k].log_fwd - lf) <= LOG_TOL * max(1, abs(lf)) and abs(fbs[k].log_bwd - lb) <= LOG_TOL * max(1, abs(lb)), (k, fbs[k].log_fwd, lf, fbs[k].log_bwd, lb)
    for fb, (f, b, sch) in zip(fbs, single):
        assert fb.log_fwd == f and fb.log_bwd == b and fb.schedule == sch
        fb.close()


def test_kernel_times_go_to_one_pair_per_launch_group(pg, monkeypatch):
    """pagan_fb_kernel_ms across a batch of every schedule (two deep pairs, of two workgroup sizes): the tiled launch, the ring
    kind and the deep kind each report their two times at exactly one pair; every other pair, the small one included, reports
    exactly 0.0 -- and the same small pair alone, as the call's only pair, is timed."""
    cases, n_deep, want_sched = _mixed_cases(monkeypatch, (0, 2), per_rep=1)
    assert n_deep == 2
    _second_size(cases, n_deep)
    fbs = pgm.full_probability_batch(cases)
    ms = [(fb.forward_ms, fb.backward_ms) for fb in fbs]
    print("kernel ms by pair:", list(zip(want_sched, ms)))
    assert [fb.schedule for fb in fbs] == want_sched
    for fb in fbs:
        fb.close()
    for sched in (1, 2, 3):
        timed = [m for m, s in zip(ms, want_sched) if s == sched and m[0] > 0 and m[1] > 0]
        assert len(timed) == 1, (sched, ms)
        assert all(m == (0.0, 0.0) for m, s in zip(ms, want_sched) if s == sched and m not in timed), (sched, ms)
    assert ms[-1] == (0.0, 0.0) and want_sched[-1] == 0, ms
    alone = pgm.FullProbability(*cases[-1])
    assert alone.schedule == 0 and alone.forward_ms > 0 and alone.backward_ms > 0, (alone.forward_ms, alone.backward_ms)
    alone.close()
