"""GPU: paths sampled on the device (dp_fb_sample.inc, pg_fb_sample: K paths per pair in one launch, a lane a path) against the
host sampler they restate (pagan_fb_sample_path on pagan_sample_uniforms_path's numbers) -- cell for cell, with no share of
paths left out --, against the oracle's sampler, and, as a distribution, against the posterior of the same pass.

Two inputs, both small enough for the oracle's dense posterior.  A: a leaf pair, full matrix of 29 x 39 cells; its paths have 38 to
56 steps, so the lanes of a wave finish at different steps.  B: nodes 4, 5, 6 of an anchored walk of eight leaves, all three
inside tunnels; nodes 5 and 6 have multi-edge sites and skipped sites.

The device's exp differs from glibc's in the last bits, which can move a pick only where total * u lies within a few ulp of a
running sum (about 1e-13 per step).  Should a fixed seed ever hit that, show the margin and change the seed, not the comparison."""
import numpy as np
import pytest

import pagan2_msa_amd as pgm
from pagan2_msa_amd import abi, host, synth

import fb_tables

pytestmark = pytest.mark.gpu
LOG_TOL = 1e-9
SEED = 5
N_REF = 200                                   # paths 0 .. 199 of every pair have a host reference


class Pair:
    def __init__(self, name, left, right, mp, band, node):
        self.name, self.left, self.right, self.mp, self.band, self.node = name, left, right, mp, band, node
        self.fb = pgm.FullProbability(left, right, mp, band)
        self.Lx, self.Ly = left.n_sites - 1, right.n_sites - 1


@pytest.fixture(scope="module")
def pairs(pg, oracle):
    """[A, B4, B5, B6] with their passes run once, and per pair the host sampler's paths 0 .. N_REF - 1 (visited cells, result)."""
    out = []
    _, seqs, _ = synth.evolve_balanced(2, 40, branch=0.15, sub=0.2, indel_start=0.05, mean_len=3, seed=71)
    gl, gr = (host.HGraph.leaf(s).flatten() for s in seqs)
    out.append(Pair("A", gl, gr, host.model_prob(1, 0.3, base_freq=[0.3, 0.2, 0.2, 0.3]), None, 3))
    assert (out[0].Lx, out[0].Ly) == (29, 39)                # (the matrices' rows and columns: 30 and 40 sites with the stop sites)
    names, seqs, nwk = synth.evolve_balanced(8, 60, branch=0.05, sub=0.05, indel_start=0.03, mean_len=3, seed=44)
    msa = host.Msa(names, seqs, nwk, use_anchors=1, prefix_hit_length=8).align()
    bf = np.array([sum(s.count(x) for s in seqs) for x in "ACGT"], np.float32)
    bf /= bf.sum()
    for k in (4, 5, 6):
        left, right, _model, band = msa.node_job(k)
        assert band is not None
        out.append(Pair("B%d" % k, left, right, host.model_prob(1, msa.node_info(k).dist, base_freq=bf), band, 8 + k))
    multi = [int((np.diff(p.left.bwd_off) > 1).sum() + (np.diff(p.right.bwd_off) > 1).sum()) for p in out]
    assert multi[2] > 0 and multi[3] > 0, multi
    # behind them (the tests above index the first four): tables of 211 and 1892 states, asymmetric, with zeros (fb_tables.py) --
    # pg_fb_sample's score lookup from memory, which a symmetric table without a zero cannot tell from its transpose
    extra = dict(fb_tables.leaf_pairs(), **fb_tables.graph_pairs())
    extra["K1892"] = fb_tables.codon_leaf_pair(oracle)
    extra["G211w"], extra["K1892g"] = fb_tables.walk_root_pair(2), fb_tables.walk_root_pair(3, oracle)
    for node, name in enumerate(("Q64z", "G211", "G211z", "K1892", "G211w", "K1892g"), 20):
        q = extra[name]
        out.append(Pair(name, q.left, q.right, q.mp, q.band, node))
        assert np.isfinite(out[-1].fb.log_fwd) and q.mp.n_states > 16
    for p in out:
        p.ref = []
        for q in range(N_REF):
            u = host.sample_uniforms_path(SEED, p.node, q, p.Lx + p.Ly + 1)
            res, visited = p.fb.sample_path(u)
            p.ref.append((res, visited, u))
        _lf, _lb, p.opost, p.ologf = oracle.fb(p.left, p.right, p.mp, band=p.band)
    yield out
    for p in out:
        p.fb.close()


@pytest.mark.parametrize("n_paths", [1, 64, 65, 200])
def test_path_for_path_against_the_host_sampler(pg, oracle, pairs, n_paths):
    """The last lane alone, a full wave, one lane of a second group, several groups: every path equals the host's."""
    for p in pairs:
        sp = p.fb.sample_paths(SEED, p.node, n_paths)
        sm = sp.summary()
        assert np.all(sm["status"] == 0), (p.name, sm["status"])
        for q in range(n_paths):
            want_res, want_vis, u = p.ref[q]
            got = sp.visited(q)
            assert np.array_equal(got, want_vis), (p.name, q)
            res = sp.result(q)
            assert res.status == 0 and res.score == p.fb.log_fwd and res.same_alignment(want_res), (p.name, q)
            assert np.array_equal(res.cols, want_res.cols) and np.array_equal(res.left_used, want_res.left_used)
            assert np.array_equal(res.right_used, want_res.right_used)
            if (p.band is not None or p.name == "K1892g") and n_paths == 200:        # B, K1892g: the oracle's sampler on the same numbers, the same cells
                ocells, _end = oracle.sample_path(p.left, p.right, p.mp, p.ologf, u)
                assert np.array_equal(got, ocells), (p.name, q)
        allv, alln = sp.visited_all()                        # one copy of the trace buffer: the same cells again
        for q in range(n_paths):
            assert alln[q] == p.ref[q][1].shape[0] and np.array_equal(allv[q, :alln[q]], p.ref[q][1]), (p.name, q)
            assert not allv[q, alln[q]:].any()
        sp.close()
    steps = [v.shape[0] for _r, v, _u in pairs[0].ref[:64]]
    assert min(steps) < max(steps)                           # (A: the lanes of a wave finish at different steps)


def _bytes(sp):
    sm = sp.summary()
    vis, n = sp.visited_all()
    return b"".join(sm[k].tobytes() for k in sorted(sm)) + vis.tobytes() + n.tobytes()


def test_batch_equals_single(pg, pairs):
    """One launch over A and B's nodes (paths of 38 to 120 steps side by side, two groups a pair): the traces and summaries
    of the single calls, byte for byte; a second call gives the same bytes.  (A call draws the same number of paths for every
    pair, so all pairs have the launch's group count: the kernel's early return for a pair with fewer groups is not exercised.)"""
    fbs, nodes = [p.fb for p in pairs], [p.node for p in pairs]
    assert len({p.Lx + p.Ly for p in pairs}) > 1
    batch = pgm.sample_paths_batch(fbs, SEED, nodes, 70)
    again = pgm.sample_paths_batch(fbs, SEED, nodes, 70)
    assert batch[0].ms > 0 and all(b.ms == 0 for b in batch[1:])            # booked at the batch's first pair
    for p, b, a in zip(pairs, batch, again):
        single = p.fb.sample_paths(SEED, p.node, 70)
        assert _bytes(b) == _bytes(single) == _bytes(a), p.name
        assert np.array_equal(b.visited(69), p.ref[69][1])
        single.close()
    other = pgm.sample_paths_batch(fbs, SEED + 1, nodes, 70)                # (and the seed matters)
    assert any(_bytes(o) != _bytes(b) for o, b in zip(other, batch))
    for s in batch + again + other:
        s.close()


def _log_q_of(p, end_state, visited):
    """A's path probability from its cells: the transition log terms of include/pagan_dp.h's model (leaf edges: log weight 0),
    end corner included, minus log_fwd."""
    lg = lambda x: float(np.log(np.float64(np.float32(x))))
    ext, opn, ng = lg(p.mp.gap_ext), lg(p.mp.gap_open), lg(p.mp.non_gap)
    total = ng if end_state == 2 else 0.0                    # the end corner: a match closes with non_gap, a gap with 1
    states = [int(v[2]) for v in visited] + [2]              # the cell behind the last visited one is (0, 0) in M
    assert end_state == states[0]
    for t, (i, j, s) in enumerate(visited):
        nxt = states[t + 1]
        if s == 2:
            sc = lg(p.mp.score[p.left.state[i], p.right.state[j]])
            total += (ng + ng if nxt == 2 else ng) + sc
        else:
            total += ext if nxt == s else (ng + opn if nxt == 2 else opn)
    return total - p.fb.log_fwd


def test_summaries(pg, pairs):
    for p in pairs:
        sp = p.fb.sample_paths(SEED, p.node, 130)
        sm = sp.summary()
        bare = p.fb.sample_paths(SEED, p.node, 130, traces=False)
        sb = bare.summary()
        for key in sm:
            assert sm[key].tobytes() == sb[key].tobytes(), (p.name, key)
        with pytest.raises(pgm.PaganError) as e:
            bare.visited(0)
        assert e.value.code == abi.PAGAN_E_ARG
        with pytest.raises(pgm.PaganError) as e:
            bare.result(0)
        assert e.value.code == abi.PAGAN_E_ARG
        bare.close()
        for q in range(130):
            v = sp.visited(q)
            assert sm["n_steps"][q] == v.shape[0]
            assert [sm["n_x"][q], sm["n_y"][q], sm["n_m"][q]] == [int((v[:, 2] == s).sum()) for s in (0, 1, 2)], (p.name, q)
            assert sm["log_q"][q] < 0
            if p.name == "A":
                want = _log_q_of(p, sp.result(q).end[0], v)
                print("A path %d: log_q %.12f from the cells %.12f" % (q, sm["log_q"][q], want))
                assert abs(sm["log_q"][q] - want) <= LOG_TOL * max(1.0, abs(want)), (q, sm["log_q"][q], want)
        sp.close()


def test_zero_entries_are_never_matched(pg, pairs):
    """The pairs under a table with zeros: every path is drawn (status 0), no path holds a match cell whose entry is 0 -- while
    the transposed entry of some matched cell is 0, so a transposed lookup would have had to refuse that step --, and on the leaf
    pairs log_q is the path's probability from the table as [left state, right state]."""
    for p in pairs:
        if p.name not in ("Q64z", "G211z", "K1892"):
            continue
        sp = p.fb.sample_paths(SEED, p.node, N_REF)
        sm = sp.summary()
        assert np.all(sm["status"] == 0), (p.name, sm["status"])
        transposed_zero = 0
        for q in range(N_REF):
            v = sp.visited(q)
            m = v[v[:, 2] == 2]
            a, b = p.left.state[m[:, 0]], p.right.state[m[:, 1]]
            assert np.all(p.mp.score[a, b] > 0), (p.name, q)
            transposed_zero += int((p.mp.score[b, a] == 0).sum())
            if p.name != "G211z":
                want = _log_q_of(p, sp.result(q).end[0], v)
                assert abs(sm["log_q"][q] - want) <= LOG_TOL * max(1.0, abs(want)), (p.name, q, sm["log_q"][q], want)
        print("%s: %d matched cells in %d paths whose transposed entry is 0" % (p.name, transposed_zero, N_REF))
        assert transposed_zero > 0 or p.name == "K1892"         # (the codon table has no zero: its asymmetry shows in log_q)
        sp.close()


@pytest.mark.parametrize("which, K, seed, node", [(0, 4096, 11, 5), (0, 4096, 12, 5), (1, 2048, 21, 12), (2, 2048, 21, 13), (3, 2048, 21, 14)])
def test_the_sampler_draws_from_the_posterior(pg, pairs, which, K, seed, node):
    """Visits of every (i, j, state) over K paths against the posterior of the same pass: |f - p| <= 5 sqrt(p (1 - p) / K) + 4 / K
    at every cell but (0, 0), which a trace never holds.  The seeds are fixed; the oracle's sampler on these numbers stays within
    2.9 standard deviations."""
    p = pairs[which]
    sp = p.fb.sample_paths(seed, node, K)
    assert np.all(sp.summary()["status"] == 0)
    vis, n = sp.visited_all()
    sp.close()
    count = np.zeros((p.Lx, p.Ly, 3))
    for q in range(K):
        v = vis[q, :n[q]]
        assert len({(int(a), int(b)) for a, b, _s in v}) == v.shape[0]           # a path visits a cell once
        np.add.at(count, (v[:, 0], v[:, 1], v[:, 2]), 1)
    f = count / K
    post = p.fb.posterior()
    assert np.allclose(post, p.opost, rtol=1e-7, atol=1e-12)
    pc = np.clip(post, 0.0, 1.0)
    bound = 5 * np.sqrt(pc * (1 - pc) / K) + 4.0 / K
    dev = np.abs(f - post)
    dev[0, 0, :] = 0
    worst = np.unravel_index(np.argmax(dev - bound), dev.shape)
    z = (np.abs(f - post) / np.maximum(np.sqrt(pc * (1 - pc) / K), 1e-300))[pc * (1 - pc) * K > 1]
    print("%s K %d: largest normalised deviation %.2f" % (p.name, K, z.max()))
    assert np.all(dev <= bound), (worst, f[worst], post[worst])


def test_zero_probability_and_arguments(pg, pairs):
    a = pairs[0]
    band = abi.Band(np.zeros(a.Lx, np.int32), np.full(a.Lx, 3, np.int32))        # the tunnel never reaches the last columns
    assert a.Ly - 1 > 3
    fb = pgm.FullProbability(a.left, a.right, a.mp, band)
    assert fb.log_fwd == -np.inf
    sp = fb.sample_paths(SEED, 3, 66)
    sm = sp.summary()
    assert np.all(sm["status"] == 1) and not sm["n_steps"].any()
    host_res, host_vis = fb.sample_path(host.sample_uniforms_path(SEED, 3, 65, a.Lx + a.Ly + 1))
    for q in (0, 63, 65):
        res = sp.result(q)
        assert res.status == abi.PAGAN_DP_UNREACHABLE and res.cols.shape[0] == 0 and res.score == -np.inf
        assert res.same_alignment(host_res) and sp.visited(q).shape[0] == host_vis.shape[0] == 0
    for q in (-1, 66):
        with pytest.raises(pgm.PaganError) as e:
            sp.visited(q)
        assert e.value.code == abi.PAGAN_E_ARG
        with pytest.raises(pgm.PaganError) as e:
            sp.result(q)
        assert e.value.code == abi.PAGAN_E_ARG
    sp.close()
    for bad in (0, -4):
        with pytest.raises(pgm.PaganError) as e:
            fb.sample_paths(SEED, 3, bad)
        assert e.value.code == abi.PAGAN_E_ARG
    import ctypes as C
    L = pgm.lib()
    out = (C.c_void_p * 2)()
    handles = (C.c_void_p * 2)(fb._h, None)
    nodes = np.array([3, 4], np.int32)
    assert L.pagan_fb_sample_paths_batch(2, handles, 1, nodes.ctypes.data_as(C.POINTER(C.c_int32)), 4, 0, out) == abi.PAGAN_E_ARG
    assert L.pagan_fb_sample_paths(fb._h, 1, 3, 4, 2, out) == abi.PAGAN_E_ARG          # an unknown flag
    assert not out[0] and not out[1]
    fb.close()


def _walk_trees():
    """the two trees of test_msa_fb_gpu.py, and four protein leaves of ~60 residues (211 states: the samplers' lookup from memory)"""
    a = synth.evolve_balanced(8, 400, branch=0.04, sub=0.04, indel_start=0.01, mean_len=4, seed=46)
    b = synth.evolve_balanced(4, 3000, branch=0.01, sub=0.01, indel_start=0.008, mean_len=4, seed=61)
    c = synth.evolve_balanced(4, 60, branch=0.08, sub=0.1, indel_start=0.03, mean_len=3, seed=57, alphabet=fb_tables.AA)
    return [(a, {"use_anchors": 0}), (b, {"use_anchors": 1}), (c, {"use_anchors": 0, "data_type": 2})]


def test_the_walk_samples_the_same_paths_on_the_device(pg):
    for (names, seqs, nwk), opts in _walk_trees():
        on_host = host.Msa(names, seqs, nwk, sample_path=1, sample_seed=1, **opts).align()
        on_dev = host.Msa(names, seqs, nwk, sample_path=1, sample_seed=1, sample_on_device=1, **opts).align()
        by_node = host.Msa(names, seqs, nwk, sample_path=1, sample_seed=1, sample_on_device=1, **opts)
        while by_node.remaining > 0:
            by_node.align_nodes(by_node.ready()[-1:])
        by_node.finish()
        assert on_dev.alignment_all() == on_host.alignment_all() == by_node.alignment_all()
        for k in range(on_host.n_internal):
            want = on_host.node_result(k)
            for walk in (on_dev, by_node):
                got = walk.node_result(k)
                assert got.status == 0 and got.same_alignment(want), k
                assert np.array_equal(got.cols, want.cols) and np.array_equal(got.left_used, want.left_used), k
                assert np.array_equal(got.right_used, want.right_used), k
                assert np.float64(walk.node_info(k).score).tobytes() == np.float64(on_host.node_info(k).score).tobytes()
                assert walk.node_support(k).tobytes() == on_host.node_support(k).tobytes(), k
                assert walk.node_fb(k)[:2] == on_host.node_fb(k)[:2] and walk.node_fb(k)[3] >= 0


def test_the_protein_walk_samples_every_node_as_the_stand_alone_chain(pg):
    """Four protein leaves of ~60 residues (211 states: the samplers' score lookup reads memory) with sample_path=1, once on the
    host sampler and once on the device's: every node of either walk is what the stand-alone chain gives on node_job(k) and
    node_model_prob(k) -- FullProbability, then sample_path on pagan_sample_uniforms(seed, n + k, ...) and path 0 of sample_paths
    under the same key --, columns, used edges, score and support."""
    names, seqs, nwk = synth.evolve_balanced(4, 60, branch=0.08, sub=0.1, indel_start=0.03, mean_len=3, seed=57, alphabet=fb_tables.AA)
    n, seed = len(names), 3
    opts = {"data_type": 2, "use_anchors": 0, "sample_path": 1, "sample_seed": seed}
    on_host = host.Msa(names, seqs, nwk, **opts).align()
    on_dev = host.Msa(names, seqs, nwk, sample_on_device=1, **opts).align()
    assert on_host.n_internal == 3 and on_host.alignment_all() == on_dev.alignment_all()
    top = 0
    for k in range(3):
        left, right, _model, band = on_host.node_job(k)
        mp = on_host.node_model_prob(k)
        assert mp.n_states == 211
        top = max(top, int(left.state[1:-1].max()), int(right.state[1:-1].max()))
        fb = pgm.FullProbability(left, right, mp, band)
        by_host, _visited = fb.sample_path(host.sample_uniforms(seed, n + k, left.n_sites + right.n_sites - 1))
        sp = fb.sample_paths(seed, n + k, 1)
        by_dev = sp.result(0)
        assert by_host.status == by_dev.status == 0 and sp.summary()["status"][0] == 0
        for walk in (on_host, on_dev):
            got = walk.node_result(k)
            for want in (by_host, by_dev):
                assert got.status == 0 and np.array_equal(got.cols, want.cols), k
                assert np.array_equal(got.left_used, want.left_used) and np.array_equal(got.right_used, want.right_used), k
            assert walk.node_info(k).score == fb.log_fwd == walk.node_fb(k)[0], k
            assert walk.node_support(k).tobytes() == fb.path_support(by_host.cols).tobytes(), k
        sp.close()
        fb.close()
    assert top >= 20                                             # (an ancestral state entered the root's pair)
