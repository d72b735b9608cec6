"""CPU: the forward/backward oracle (oracle/oracle_fb.cpp) pinned by a second, exact reading (tests/pycheck_fb.py: memoised path
sums over the reference's transitions in 50-digit decimals).  test_fb_cpu.py compares the oracle's two arithmetics, which are one
set of loops; a wrong loop passes it.  Here every log forward cell, both totals and every posterior of the oracle, in both
arithmetics, must equal the exact values: logs to 1e-12 (a double log-sum-exp adds a few ulp per cell diagonal, there are at most
200 diagonals, 2e-16 each: two orders of margin), posteriors to the project's 1e-7 relative + 1e-12 absolute; the -inf cells
must be the same set.  Every test prints its measured worst case."""
import numpy as np
import pytest

from pagan2_msa_amd import abi, host, synth

import pycheck_fb
from fb_testlib import random_tunnel

LOG_TOL = 1e-12


def against_exact(oracle, left, right, mp, band=None, what=""):
    """oracle.fb in both arithmetics against the exact pass; returns the exact results and the worst differences
    (logs: |a - b| / max(1, |b|); posteriors: absolute)."""
    r = pycheck_fb.run(left, right, mp, band)
    assert pycheck_fb.consistent(r["exact"]), what
    worst_log = worst_post = 0.0
    for log_space in (True, False):
        lf, lb, post, logf = oracle.fb(left, right, mp, band=band, log_space=log_space)
        for got, want in ((lf, r["log_fwd"]), (lb, r["log_bwd"])):
            if np.isinf(want):
                assert got == want, (what, log_space, got, want)
            else:
                worst_log = max(worst_log, abs(got - want) / max(1.0, abs(want)))
        fin = np.isfinite(r["log_f"])
        assert np.array_equal(fin, np.isfinite(logf)) and not np.isnan(logf).any(), (what, log_space)
        assert np.all(np.isneginf(logf[~fin])), (what, log_space)
        if fin.any():
            worst_log = max(worst_log, float((np.abs(logf[fin] - r["log_f"][fin]) / np.maximum(1.0, np.abs(r["log_f"][fin]))).max()))
        assert not np.isnan(post).any(), (what, log_space)
        worst_post = max(worst_post, float(np.abs(post - r["posterior"]).max()))
        assert np.allclose(post, r["posterior"], rtol=1e-7, atol=1e-12), (what, log_space)
    assert worst_log <= LOG_TOL, (what, worst_log)
    return r, worst_log, worst_post


def hand_pair():
    lg = lambda w: np.log(np.float32(w))
    left = abi.Graph([-1, 0, -1], [0, 0, 1, 3], [0, 1, 0], [0, 0, lg(0.25)], [1, 2, 3], n_edges=4)
    right = abi.Graph([-1, 0, 1, -1], [0, 0, 1, 2, 4], [0, 1, 2, 1], [0, 0, 0, lg(0.5)], [1, 2, 3, 4], n_edges=5)
    mp = abi.ModelProb(np.array([[0.5, 0.25], [0.125, 0.125]], np.float32), 0.125, 0.5, 0.75)
    return left, right, mp


HAND_PATHS = [  # (cells behind the start corner M(0,0), start -> end; weight up to the last cell; end weight; times the forward end corner counts it)
    ([(1, 0, 0), (1, 1, 1), (1, 2, 1)], 0.75 * 0.125 * 0.125 * 0.5, 1.0, 1),
    ([(1, 0, 0), (1, 1, 1)], 0.75 * 0.125 * 0.125, 1.0, 2),
    ([(0, 1, 1), (1, 1, 0), (1, 2, 1)], 0.75 * 0.125 * 0.125 * 0.125, 1.0, 1),
    ([(0, 1, 1), (0, 2, 1), (1, 2, 0)], 0.75 * 0.125 * 0.5 * 0.125, 1.0, 1),
    ([(0, 1, 1), (1, 2, 2)], 0.75 * 0.125 * 0.75 * 0.25, 0.75, 1),
    ([(1, 1, 2), (1, 2, 1)], 0.75 * 0.75 * 0.5 * 0.75 * 0.125, 1.0, 1),
    ([(1, 1, 2)], 0.75 * 0.75 * 0.5, 0.75 * 0.5, 1),
]


def test_hand_worked_vector(oracle):
    """Left: start, one site L1 (state 0), end; edges start -> L1 -> end and a second end edge start -> end of weight 0.25.
    Right: start, R1 (state 0), R2 (state 1), end; edges start -> R1 -> R2 -> end and a second end edge R1 -> end of weight 0.5.
    Model: non_gap 0.75, gap_open 0.125, gap_ext 0.5, gap_close 1; score(L1, R1) = 0.5, score(L1, R2) = 0.25.  Cells (i, j) with
    i in {0, 1}, j in {0, 1, 2}.  Transitions: into X or Y from the same gap 0.5, from the other gap 0.125, from M 0.75 * 0.125;
    into M from M 0.75 * 0.75 * score, from a gap 0.75 * score, times both edges' weights (all 1 inside the matrices here).
    The ends: left end edges from sites [1, 0], right end edges from sites [2, 1]; a path ends from M(p, q) with 0.75 * weights,
    from X(p, 2) or Y(1, q) with 1.  All paths that reach an end, from M(0,0):

      1  X(1,0) Y(1,1) Y(1,2)   0.09375 * 0.125 * 0.5    = 0.005859375     Y-close, first right edge: once
      2  X(1,0) Y(1,1)          0.09375 * 0.125          = 0.01171875      Y-close, second right edge: once per left edge = twice
      3  Y(0,1) X(1,1) Y(1,2)   0.09375 * 0.125 * 0.125  = 0.00146484375   Y-close, once
      4  Y(0,1) Y(0,2) X(1,2)   0.09375 * 0.5 * 0.125    = 0.005859375     X-close, once
      5  Y(0,1) M(1,2)          0.09375 * 0.75 * 0.25    = 0.017578125     M end 0.75
      6  M(1,1) Y(1,2)          0.28125 * 0.09375        = 0.0263671875    Y-close, once
      7  M(1,1)                 0.75 * 0.75 * 0.5        = 0.28125         M end over R1 -> end: 0.75 * 0.5

    (X(0, .) and M(0, .), M(., 0) have no way in, so the ends from X(0,2), M(0,2), M(0,1) carry nothing.)
    Backward total = 1 + 2 + 3 + 4 + 0.75 * 5 + 6 + 0.375 * 7 = 0.169921875; forward total = that + path 2 once more = 0.181640625.
    (The weight 0.5 enters as exp(float(log(0.5))), which is 0.5 (1 - 2e-9): the comparison allows 1e-8.)"""
    left, right, mp = hand_pair()
    bwd = sum(w * e for _c, w, e, _n in HAND_PATHS)
    fwd = sum(w * e * n for _c, w, e, n in HAND_PATHS)
    assert abs(bwd - 0.169921875) < 1e-15 and abs(fwd - 0.181640625) < 1e-15
    r, worst_log, worst_post = against_exact(oracle, left, right, mp, what="hand")
    print("hand vector: oracle against exact: logs %.3g, posteriors %.3g" % (worst_log, worst_post))
    assert abs(r["log_fwd"] - np.log(fwd)) < 1e-8 and abs(r["log_bwd"] - np.log(bwd)) < 1e-8
    # the posterior and the visit probability of every cell from the list
    post, visit = np.zeros((2, 3, 3)), np.zeros((2, 3, 3))
    post[0, 0, 2] = bwd / fwd
    visit[0, 0, 2] = 1.0
    for cells, w, e, n in HAND_PATHS:
        for i, j, s in cells:
            post[i, j, s] += w * e / fwd
            visit[i, j, s] += w * e * n / fwd
    assert np.allclose(r["posterior"], post, rtol=1e-8, atol=1e-15) and np.allclose(r["visit_prob"], visit, rtol=1e-8, atol=1e-15)
    assert abs(r["visit_prob"][1, 1, 1] - r["posterior"][1, 1, 1] - 0.01171875 / fwd) < 1e-9     # path 2's Y-close counted twice
    # path_log_prob of every path; over all paths, each as often as the end corner lists it, the probabilities sum to 1
    ex = r["exact"]
    total = 0.0
    for cells, w, e, n in HAND_PATHS:
        back = cells[::-1]
        lp = ex.path_log_prob(np.array(back), (back[0][2], back[0][0], back[0][1]))
        assert abs(lp - np.log(w * e / fwd)) < 1e-8
        total += n * np.exp(lp)
    assert abs(total - 1) < 1e-12
    with pytest.raises(ValueError):
        ex.path_log_prob(np.array([(1, 2, 1), (1, 0, 0)]), (1, 1, 2))           # Y(1,2) has no transition from X(1,0)


def test_the_oracle_sampler_draws_the_hand_vector_paths_as_often_as_the_exact_reading_says(oracle):
    """4,000 paths of oracle.sample_path on the hand vector: every path is one of the seven, and path k comes with frequency
    n_k * exp(path_log_prob) within 5 sqrt(p (1 - p) / K) + 4 / K (path 2, whose end the corner lists twice, twice as often as its
    single pick's probability)."""
    left, right, mp = hand_pair()
    ex = pycheck_fb.Exact(left, right, mp)
    _lf, _lb, _post, logf = oracle.fb(left, right, mp)
    rng = np.random.default_rng(12)
    K = 4000
    seen = {}
    for _ in range(K):
        cells, end = oracle.sample_path(left, right, mp, logf, rng.random(left.n_sites + right.n_sites))
        key = tuple(map(tuple, cells.tolist()))
        if key not in seen:
            seen[key] = [0, ex.path_log_prob(cells, end)]
        seen[key][0] += 1
    want = {tuple(c[::-1]): n for c, _w, _e, n in HAND_PATHS}
    assert set(seen) <= set(want)
    worst = 0.0
    for key, n in want.items():
        count, lp = seen.get(key, [0, None])
        if lp is None:
            lp = ex.path_log_prob(np.array(key), (key[0][2], key[0][0], key[0][1]))
        p = n * np.exp(lp)
        sd = np.sqrt(p * (1 - p) / K)
        worst = max(worst, abs(count / K - p) / sd)
        assert abs(count / K - p) <= 5 * sd + 4.0 / K, (key, count, p)
    print("hand vector: largest deviation of the oracle's sampler %.2f standard deviations" % worst)


def tiny_pair(seed):
    p_dead = 0.15 if seed % 2 else 0.0
    left = synth.random_graph(3 + seed % 6, 4, 300 + seed, p_extra=0.5, max_span=4, p_dead=p_dead)
    right = synth.random_graph(2 + seed % 5, 4, 1300 + seed, p_extra=0.5, max_span=4, p_dead=p_dead)
    return left, right


def test_tiny_random_graph_pairs(oracle):
    """40 pairs of 3-10 sites from synth.random_graph (degree up to 4 in shuffled order, spans up to 5, weights != 1, half of them
    with predecessor-less sites).  Conditions on the inputs: at least 4 have total probability 0, at least 3 have a forward
    total above the backward total (multi-edge end sites on both sides)."""
    mp = oracle.model_prob(1, 0.1, base_freq=[0.3, 0.2, 0.2, 0.3])
    zero = differ = 0
    worst_log = worst_post = 0.0
    for seed in range(40):
        left, right = tiny_pair(seed)
        r, wl, wp = against_exact(oracle, left, right, mp, what="tiny %d" % seed)
        worst_log, worst_post = max(worst_log, wl), max(worst_post, wp)
        if np.isinf(r["log_fwd"]):
            zero += 1
            assert r["log_fwd"] == r["log_bwd"] == -np.inf and not r["posterior"].any() and not r["visit_prob"].any()
        else:
            assert r["log_fwd"] >= r["log_bwd"] - 1e-12
            differ += r["log_fwd"] - r["log_bwd"] > 1e-6
    print("tiny pairs: %d with total 0, %d with log_fwd != log_bwd; oracle against exact: logs %.3g, posteriors %.3g"
          % (zero, differ, worst_log, worst_post))
    assert zero >= 4 and differ >= 3, (zero, differ)


MID = [  # (left sites, right sites, max_span, p_dead, tunnel half-widths or None, data type)
    (70, 64, 14, 0.0, None, 1),
    (84, 90, 20, 0.02, (6, 20), 1),
    (100, 76, 17, 0.0, (6, 20), 1),
    (62, 80, 20, 0.02, None, 1),
    (66, 72, 16, 0.0, (6, 20), 2),
    (90, 60, 14, 0.0, None, 1),
]


@pytest.mark.parametrize("case", range(len(MID)))
def test_random_graph_pairs_of_60_to_100_sites(oracle, case):
    nl, nr, span, p_dead, halves, data_type = MID[case]
    mp = oracle.model_prob(1, 0.1, base_freq=[0.3, 0.2, 0.2, 0.3]) if data_type == 1 else oracle.model_prob(2, 0.2)
    assert mp.n_states == (15 if data_type == 1 else 211)
    n_states = 4 if data_type == 1 else 211
    left = synth.random_graph(nl, n_states, 40 + case, p_extra=0.4, max_deg=4, max_span=span, p_dead=p_dead)
    right = synth.random_graph(nr, n_states, 60 + case, p_extra=0.4, max_deg=4, max_span=span, p_dead=p_dead)
    band = random_tunnel(np.random.default_rng(case), nl + 1, nr + 1, *halves) if halves else None
    r, worst_log, worst_post = against_exact(oracle, left, right, mp, band, what="mid %d" % case)
    print("pair %d (%d x %d, span %d, %s): log_fwd %.12g log_bwd %.12g; oracle against exact: logs %.3g, posteriors %.3g"
          % (case, nl, nr, span, "tunnel" if band else "full", r["log_fwd"], r["log_bwd"], worst_log, worst_post))
    assert np.isfinite(r["log_fwd"])                           # (these pairs are about the sums; the zero totals are above and below)
    if band is not None:
        outside = np.ones((nl + 1, nr + 1), bool)
        for i in range(nl + 1):
            outside[i, band.upper[i]:band.lower[i] + 1] = False
        assert outside.any() and np.all(np.isneginf(r["log_f"][outside])) and not r["posterior"][outside].any()


def test_plain_leaf_pair(oracle):
    _, seqs, _ = synth.evolve_balanced(2, 60, branch=0.1, sub=0.1, indel_start=0.03, mean_len=3, seed=8)
    left, right = (host.HGraph.leaf(s).flatten() for s in seqs)
    mp = oracle.model_prob(1, 0.2, base_freq=[0.25] * 4)
    r, worst_log, worst_post = against_exact(oracle, left, right, mp, what="leaves")
    print("leaf pair %d x %d: oracle against exact: logs %.3g, posteriors %.3g" % (left.n_sites - 1, right.n_sites - 1, worst_log, worst_post))
    assert abs(r["log_fwd"] - r["log_bwd"]) < 1e-13 * abs(r["log_fwd"])     # one end edge a side: nothing is counted twice
    assert np.allclose(r["visit_prob"], r["posterior"], rtol=1e-12, atol=0)


def test_sampled_paths_of_the_oracle_are_paths_of_the_exact_reading(oracle):
    """oracle.sample_path on 200 uniform vectors for two small random-graph pairs.  The oracle does not expose its picks'
    probabilities, so what is checked here is that every returned trace is a chain of the exact reading's transitions from the
    start corner to an end the corner lists (path_log_prob raises otherwise) and that the distinct paths' probabilities, each
    times the number of end candidates on its cell, do not exceed 1; the picks' own sum against path_log_prob is
    test_fb_exact_gpu.py's (summary()["log_q"])."""
    mp = oracle.model_prob(1, 0.1, base_freq=[0.3, 0.2, 0.2, 0.3])
    for seed in (4, 10):
        left, right = tiny_pair(seed)
        ex = pycheck_fb.Exact(left, right, mp)
        assert np.isfinite(ex.log_fwd)
        _lf, _lb, _post, logf = oracle.fb(left, right, mp)
        rng = np.random.default_rng(seed)
        mass = {}
        for _ in range(200):
            cells, end = oracle.sample_path(left, right, mp, logf, rng.random(left.n_sites + right.n_sites))
            assert cells.shape[0] == 0 or tuple(cells[0]) == (end[1], end[2], end[0])
            lp = ex.path_log_prob(cells, end)
            assert lp <= 1e-12
            first = (int(end[1]), int(end[2]), int(end[0]))
            mass[tuple(map(tuple, cells.tolist())) + (first,)] = np.exp(lp) * sum(1 for c, _w in ex.end_forward if c == first)
        print("tiny pair %d: %d distinct paths in 200 draws hold %.4f of the probability" % (seed, len(mass), sum(mass.values())))
        assert len(mass) > 1 and sum(mass.values()) <= 1 + 1e-12


def test_a_pair_with_total_zero_has_posterior_zero_in_the_oracle(oracle):
    """oracle_fb.cpp used to return exp(-inf + b - (-inf)) = NaN in every cell here; the product's fb_pexp (dp_fb_post.inc)
    returns 0, and so does the exact reading.  Two ways to a total of 0: a tunnel that misses the end corner's cells, and
    predecessor-less sites across every path."""
    mp = oracle.model_prob(1, 0.1, base_freq=[0.25] * 4)
    left = synth.random_graph(12, 4, 1, p_extra=0.5, max_span=4)
    right = synth.random_graph(14, 4, 2, p_extra=0.5, max_span=4)
    band = abi.Band(np.zeros(13, np.int32), np.full(13, 3, np.int32))
    dead = None
    for seed in range(40):
        cand = tiny_pair(seed)
        if seed % 2 and np.isinf(pycheck_fb.Exact(cand[0], cand[1], mp).log_fwd):
            dead = cand
            break
    assert dead is not None
    for l, r, b in ((left, right, band), (dead[0], dead[1], None)):
        for log_space in (True, False):
            lf, lb, post, logf = oracle.fb(l, r, mp, band=b, log_space=log_space)
            assert lf == -np.inf and lb == -np.inf
            assert not np.isnan(post).any() and not post.any() and not np.isnan(logf).any()
            assert logf[0, 0, 2] == 0.0                           # (the forward matrix itself is not empty)
        ex = pycheck_fb.run(l, r, mp, b)
        assert ex["log_fwd"] == ex["log_bwd"] == -np.inf and not ex["posterior"].any()
