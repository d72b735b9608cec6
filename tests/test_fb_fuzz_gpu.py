"""GPU: the forward/backward schedules on random graphs (synth.random_graph: degree up to 4 in shuffled list order, spans up to 71,
edge weights != 1, predecessor-less sites) of 150-300 sites -- too large for the exact reading, cheap for the oracle, which
test_pycheck_fb_cpu.py pins to the exact reading -- at the size where every operand source of the kernels is hit:

  * pg_fb_forward_tiled's fetch (dp_fb.hip; block origins at multiples of FB_T = 64) reads a predecessor from the ring of the last
    FB_RING = 12 diagonals inside the block, from memory for a cell of the block that left the ring, from the FB_H = 8 deep halo
    above the block (with its corner), from the halo left of it, and from memory for any other block.  operand_classes() sorts every
    predecessor read of a full-matrix pair into these six from the graphs alone; all six must occur between live cells;
  * the deep ring's far cells (an operand D or more diagonals back, D = 4,096 / B): there must be far cells at D = 64, 32 and 16, and
    far edges at multi-edge sites.

Where a pair misses a condition, the generator's parameters change, not the assertion.  Tolerances: test_fb_gpu.py's (1e-9 on logs,
1e-7 relative + 1e-12 absolute on posteriors, 1e-12 per in-band cell on the marginals).  Every run asserts its schedule."""
import numpy as np
import pytest

import pagan2_msa_amd as pgm
from pagan2_msa_amd import host, synth

from fb_testlib import ENV_VARS, in_band, random_tunnel, set_env

pytestmark = pytest.mark.gpu
LOG_TOL = 1e-9
FB_T, FB_RING, FB_H = 64, 12, 8                # dp_fb.hip
CLASSES = ("ring", "block beyond the ring", "halo above", "halo corner", "halo left", "another block")
HALVES = {"narrow": (5, 12), "mid": (20, 70), "b128": (70, 125), "wide": (100, 180)}

# (left sites, right sites, max_span, p_dead, data type, seed); the seeds with p_dead > 0 were chosen on the CPU for a finite total
PAIRS = [
    (150, 141, 20, 0.02, 1, 3),
    (151, 160, 6, 0.0, 1, 2),
    (170, 150, 70, 0.0, 1, 3),
    (200, 190, 20, 0.0, 1, 4),
    (190, 230, 70, 0.02, 1, 20),
    (160, 155, 6, 0.02, 1, 21),
    (301, 281, 70, 0.0, 1, 7),
    (257, 150, 20, 0.02, 1, 8),
    (180, 260, 6, 0.0, 1, 9),
    (165, 175, 20, 0.0, 2, 10),
    (230, 215, 70, 0.0, 1, 11),
    (150, 300, 20, 0.02, 1, 12),
]

# (tunnel or None, environment, schedule); "full" pairs wider than 256 cells take the blocks by default
RUNS = [
    (None, {"PAGAN_FB_GROUPS": "4"}, 1),
    (None, {"PAGAN_FB_GROUPS": "1"}, 0),
    ("narrow", {"PAGAN_FB_BAND_MIN_ND": "0"}, 1),
    ("mid", {"PAGAN_FB_BAND_MIN_ND": "0"}, 1),
    ("narrow", {"PAGAN_FB_DEEP_MIN_ND": "0"}, 3),
    ("mid", {"PAGAN_FB_DEEP_MIN_ND": "0"}, 3),
    ("b128", {"PAGAN_FB_DEEP_MIN_ND": "0"}, 3),
    ("wide", {"PAGAN_FB_DEEP_MIN_ND": "0"}, 3),
]


def make_pair(nl, nr, max_span, p_dead, data_type, seed):
    """(left, right, model_prob, {tunnel name: Band}) -- host only, from synth and the seed alone"""
    n_states = 4 if data_type == 1 else 211
    left = synth.random_graph(nl, n_states, 7000 + seed, p_extra=0.4, max_deg=4, max_span=max_span, p_dead=p_dead)
    right = synth.random_graph(nr, n_states, 8000 + seed, p_extra=0.4, max_deg=4, max_span=max_span, p_dead=p_dead)
    mp = host.model_prob(1, 0.1, base_freq=[0.3, 0.2, 0.2, 0.3]) if data_type == 1 else host.model_prob(2, 0.2)
    rng = np.random.default_rng(9000 + seed)
    bands = {name: random_tunnel(rng, nl + 1, nr + 1, *h) for name, h in HALVES.items()}
    return left, right, mp, bands


def edges_of(g, n):
    """(dst, src) of the bwd edges of the sites 1 .. n - 1 (the matrix's rows or columns)"""
    dst = np.repeat(np.arange(g.n_sites), np.diff(g.bwd_off))
    keep = (dst >= 1) & (dst < n)
    return dst[keep].astype(np.int64), g.bwd_src[:g.bwd_off[-1]][keep].astype(np.int64)


def classify(i, j, p, q):
    """the class (index into CLASSES) of the read of (p, q) by cell (i, j) in pg_fb_forward_tiled's fetch; arrays or scalars"""
    i, j, p, q = np.broadcast_arrays(i, j, p, q)
    i0, j0, d = i // FB_T * FB_T, j // FB_T * FB_T, i + j
    out = np.full(i.shape, 5, np.int64)
    inside = (p >= i0) & (q >= j0)
    above = (p < i0) & (p >= i0 - FB_H) & (q >= j0 - FB_H)
    out[(p >= i0) & (q < j0) & (q >= j0 - FB_H)] = 4
    out[above & (q < j0)] = 3
    out[above & (q >= j0)] = 2
    out[inside & (d - (p + q) >= FB_RING)] = 1
    out[inside & (d - (p + q) < FB_RING)] = 0
    return out


def operand_classes(left, right, live):
    """reads per class over a full matrix: the X reads (p, j), the Y reads (i, q) and the M reads (p, q) of every live cell (i, j)
    whose operand cell is live too (live: [Lx, Ly] bool)"""
    Lx, Ly = live.shape
    li, lp = edges_of(left, Lx)
    rj, rq = edges_of(right, Ly)
    count = np.zeros(6, np.int64)
    cols, rows = np.arange(Ly), np.arange(Lx)
    for i, p in zip(li, lp):
        ok = live[i] & live[p]
        count += np.bincount(classify(i, cols[ok], p, cols[ok]), minlength=6)                     # X
        ok = live[i, rj] & live[p, rq]
        count += np.bincount(classify(i, rj[ok], p, rq[ok]), minlength=6)                         # M
    for j, q in zip(rj, rq):
        ok = live[:, j] & live[:, q]
        count += np.bincount(classify(rows[ok], j, rows[ok], q), minlength=6)                     # Y
    return count


def far_meets_multi(g, D):
    """sites with more than one edge of which one reaches D or further back"""
    off = g.bwd_off.astype(np.int64)
    return sum(1 for i in range(1, g.n_sites - 1) if off[i + 1] - off[i] > 1 and int(i - g.bwd_src[off[i]:off[i + 1]].min()) >= D)


def compare(fb, want, inb, what):
    """one finished pass against (log_fwd, log_bwd, posterior, log_f) of the oracle"""
    lf, lb, post, logf = want
    for got, ref in ((fb.log_fwd, lf), (fb.log_bwd, lb)):
        if np.isinf(ref):
            assert got == ref, (what, got, ref)
        else:
            assert abs(got - ref) <= LOG_TOL * max(1.0, abs(ref)), (what, got, ref)
    got = fb.log_forward()
    fin = np.isfinite(logf)
    assert not np.isnan(got).any() and np.array_equal(np.isfinite(got), fin), what
    assert np.allclose(got[fin], logf[fin], rtol=LOG_TOL, atol=LOG_TOL), (what, np.abs(got[fin] - logf[fin]).max())
    gp = fb.posterior()
    assert not np.isnan(gp).any() and np.allclose(gp, post, rtol=1e-7, atol=1e-12), (what, np.abs(gp - post).max())
    mg = fb.site_marginals()
    for side, (gap, match, state) in enumerate((("pX", "pM_left", 0), ("pY", "pM_right", 1))):
        n = inb.sum(1 - side)
        for key, ref in ((gap, post[:, :, state].sum(1 - side)), (match, post[:, :, 2].sum(1 - side))):
            assert np.all(np.abs(mg[key] - ref) <= 1e-7 * np.abs(ref) + 1e-12 * n), (what, key, np.abs(mg[key] - ref).max())


class InputCondition(AssertionError):
    """a pair that fb_route does not give to the schedule a run is meant for: a condition on the input, not a result"""


def run_pair(oracle, spec, setenv, runs=RUNS):
    """Every run of one pair; returns what the input conditions are judged on -- the operand classes of the full matrix (None when
    `runs` has no full-matrix run) and [(min_D, far cells, far edges at multi-edge sites)] of the deep-ring runs -- and the
    oracle's log_fwd of the first run."""
    left, right, mp, bands = make_pair(*spec)
    Lx, Ly = left.n_sites - 1, right.n_sites - 1
    wants, deep = {}, []
    classes = None
    for tunnel, env, schedule in runs:
        band = bands[tunnel] if tunnel else None
        if tunnel not in wants:
            wants[tunnel] = oracle.fb(left, right, mp, band=band)
        setenv(env)
        what = (spec, tunnel, env)
        code, info = pgm.fb_route(left, right, band)
        if code != schedule:
            raise InputCondition((what, "routes to schedule %d, not %d" % (code, schedule), info))
        fb = pgm.FullProbability(left, right, mp, band)
        assert fb.schedule == schedule, (what, fb.schedule)
        compare(fb, wants[tunnel], in_band(Lx, Ly, band), what)
        fb.close()
        if schedule == 3:
            D = info["min_D"]
            deep.append((D, info["far_cells"], far_meets_multi(left, D) + far_meets_multi(right, D) if info["far_cells"] else 0))
        if tunnel is None and classes is None:
            classes = operand_classes(left, right, np.isfinite(wants[None][3]).any(axis=2))
    return classes, deep, wants[runs[0][0]][0]


def sweep(oracle, n_cases, seed0, runs=RUNS):
    """tests/diagnostics/sweep_fb.py --random-graphs: the same comparison over fresh seeds.  Stops at the first mismatch (returns
    the number of mismatches, 0 or 1): nothing runs on the device after one.  A fresh pair that fb_route does not give to the
    schedule a run expects is not a mismatch: it is reported as a skipped input and the sweep goes on.  A pair whose total is 0
    (p_dead = 0.02 allows it) is compared like any other: -inf totals, posterior 0."""
    import os
    rng = np.random.default_rng(seed0)
    skipped = 0

    def setenv(env):
        for v in ENV_VARS:
            os.environ.pop(v, None)
        os.environ.update(env)
    for case in range(n_cases):
        spec = (int(rng.integers(150, 301)), int(rng.integers(150, 301)), int(rng.choice([6, 20, 70])), float(rng.choice([0.0, 0.02])),
                2 if case % 8 == 7 else 1, seed0 + case)
        try:
            classes, deep, log_fwd = run_pair(oracle, spec, setenv, runs)
        except InputCondition as e:
            skipped += 1
            print("SKIPPED INPUT case %d %s: %s" % (case, spec, str(e)[:400]), flush=True)
            continue
        except AssertionError as e:
            print("MISMATCH case %d %s: %s" % (case, spec, str(e)[:400]), flush=True)
            return 1
        print("case %d %s: log_fwd %.9g%s reads per class %s deep runs %s" % (case, spec, log_fwd, " (total 0)" if np.isinf(log_fwd) else "",
                                                                             classes.tolist() if classes is not None else None, deep), flush=True)
    print("%d of %d cases skipped as inputs" % (skipped, n_cases), flush=True)
    return 0


@pytest.mark.parametrize("k", range(len(PAIRS)))
def test_random_graph_pair_on_every_schedule(pg, oracle, monkeypatch, k):
    spec = PAIRS[k]
    classes, deep, log_fwd = run_pair(oracle, spec, lambda env: set_env(monkeypatch, env))
    print("pair %d %s: log_fwd %.9g; reads per class %s; deep runs (min_D, far cells, far at multi-edge sites) %s"
          % (k, spec, log_fwd, dict(zip(CLASSES, classes.tolist())), deep))
    assert np.isfinite(log_fwd), spec                          # (a condition on the seed)
    assert all(classes[c] > 0 for c in (0, 2, 3, 4)), classes  # every pair: the ring, both halos and the corner
    if spec[2] >= 20:
        assert classes[1] > 0 and classes[5] > 0, classes      # spans beyond 12 diagonals and beyond the halo


def test_wide_pair_takes_the_blocks_by_default(pg, oracle, monkeypatch):
    """301 x 281: the widest diagonal has more than 256 cells, so the default route is the block schedule."""
    spec = PAIRS[6]
    left, right, mp, _bands = make_pair(*spec)
    set_env(monkeypatch, {})
    code, info = pgm.fb_route(left, right, None)
    assert info["widest"] > 256 and code == 1, (code, info)
    fb = pgm.FullProbability(left, right, mp, None)
    assert fb.schedule == 1 and fb.groups > 1
    compare(fb, oracle.fb(left, right, mp), in_band(left.n_sites - 1, right.n_sites - 1, None), spec)
    fb.close()


def test_the_pairs_reach_every_operand_source(pg, oracle, monkeypatch):
    """Conditions on the inputs, from the graphs and fb_route alone (no kernel runs): over all pairs every class of read occurs
    between live cells, and the deep-ring runs have far cells at D = 64, 32 and 16, some at multi-edge sites."""
    total = np.zeros(6, np.int64)
    far = {}
    multi = 0
    set_env(monkeypatch, {"PAGAN_FB_DEEP_MIN_ND": "0"})
    for spec in PAIRS:
        left, right, mp, bands = make_pair(*spec)
        total += operand_classes(left, right, np.isfinite(oracle.fb(left, right, mp)[3]).any(axis=2))
        for name, band in bands.items():
            code, info = pgm.fb_route(left, right, band)
            assert code == 3, (spec, name, code, info)
            far[info["min_D"]] = far.get(info["min_D"], 0) + info["far_cells"]
            if info["far_cells"]:
                multi += far_meets_multi(left, info["min_D"]) + far_meets_multi(right, info["min_D"])
    print("reads per class", dict(zip(CLASSES, total.tolist())), "| far cells per min_D", far, "| far edges at multi-edge sites", multi)
    assert np.all(total > 0), dict(zip(CLASSES, total.tolist()))
    assert all(far.get(D, 0) > 0 for D in (16, 32, 64)), far
    assert multi > 0
