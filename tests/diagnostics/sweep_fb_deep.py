"""Diagnostic: a randomized sweep of the deep-ring forward/backward sweeps (dp_fb_deep.inc; schedule 3) against the oracle: the
internal nodes above the leaves of random trees (4 to 16 leaves, random lengths and divergence) behind random tunnels -- random
half-widths from a few columns to ~200, and boxes that make the ring change shape inside a pair --, every cell of the forward
matrix and every posterior, the totals to 1e-9.  A pair that does not route to schedule 3 is reported and counts as a failure
unless it is not eligible by its shape (a diagonal wider than 1,024 cells).
Usage: sweep_fb_deep.py [trees] (PG_SWEEP_SEED: another seed; --route-only: no GPU, the walk runs on the oracle's DP and only the
routing and the plans are printed; --random-graphs: instead, the deep-ring runs of tests/test_fb_fuzz_gpu.py -- synth.random_graph pairs
of 150-300 sites behind four ranges of tunnels -- over fresh seeds, stopping at the first mismatch)."""
import ctypes as C
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
import pagan2_msa_amd as pg
from pagan2_msa_amd import abi, host, synth
import oracle

oracle.build()
args = [a for a in sys.argv[1:] if not a.startswith("--")]
route_only = "--route-only" in sys.argv
n_trees = int(args[0]) if args else 6
seed0 = int(os.environ.get("PG_SWEEP_SEED", "7000"))
os.environ["PAGAN_FB_DEEP_MIN_ND"] = "0"
if "--random-graphs" in sys.argv:
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import test_fb_fuzz_gpu as fuzz
    failed = fuzz.sweep(oracle, n_trees, seed0, [r for r in fuzz.RUNS if r[2] == 3])
    print("sweep_fb_deep --random-graphs: seed %d, %d cases asked for: %s" % (seed0, n_trees, "MISMATCH" if failed else "all equal"))
    sys.exit(1 if failed else 0)
TOL = 1e-9
bad = 0
seen = {"pairs": 0, "far_pairs": 0, "segments>1": 0, "min_D": set()}


def close_logs(a, b):
    fa, fb = np.isfinite(a), np.isfinite(b)
    return np.array_equal(fa, fb) and np.allclose(a[fa], b[fb], rtol=TOL, atol=TOL)


def oracle_backend():
    L = oracle.lib()

    def fn(n, jobs, o, out, user):
        for k in range(n):
            j = jobs[k]
            rc = L.oracle_dp_align(j.left, j.right, j.model, j.band if j.band else None, o, C.byref(out[k]))
            if rc != 0:
                return rc
        return 0
    return fn


def tunnel(rng, Lx, Ly):
    half = rng.integers(3, int(rng.choice([10, 40, 90, 200])), Lx)
    centre = np.arange(Lx) * (Ly - 1) // max(Lx - 1, 1)
    upper = np.maximum.accumulate(np.maximum(centre - half, 0))
    lower = np.maximum.accumulate(np.minimum(centre + half, Ly - 1))
    for _ in range(int(rng.integers(0, 3))):                      # boxes
        a = int(rng.integers(5, max(6, Lx - 300))); rows = int(rng.integers(20, 600)); jump = int(rng.integers(20, 600))
        b = min(a + rows, Lx - 1)
        upper[a:b] = upper[a]; lower[a:b] = min(lower[b - 1] + jump, Ly - 1)
    upper = np.maximum.accumulate(upper); lower = np.maximum.accumulate(lower)
    upper[0] = 0; lower[-1] = Ly - 1
    return abi.Band(upper.astype(np.int32), lower.astype(np.int32))


def is_plain(g):
    n = g.n_sites
    return bool(np.all(np.diff(g.bwd_off)[1:] == 1) and np.array_equal(g.bwd_src[:n - 1], np.arange(n - 1)))


for tree in range(n_trees):
    rng = np.random.default_rng(seed0 + tree)
    leaves = int(rng.choice([4, 8, 16]))
    length = int(rng.integers(200, 1600 if leaves < 16 else 600))
    div = float(rng.choice([0.02, 0.04, 0.06]))
    names, seqs, nwk = synth.evolve_balanced(leaves, length, branch=div, sub=div, indel_start=0.01, mean_len=4, seed=seed0 + tree)
    msa = host.Msa(names, seqs, nwk, use_anchors=0)
    if route_only:
        keep = oracle_backend()
        msa.set_batch_backend(keep)
    msa.align()
    bf = np.array([sum(s.count(x) for s in seqs) for x in "ACGT"], np.float32)
    bf /= bf.sum()
    for k in range(msa.n_internal):
        left, right, _m, _b = msa.node_job(k)
        if is_plain(left) and is_plain(right):
            continue
        mp = host.model_prob(1, msa.node_info(k).dist, base_freq=bf)
        band = tunnel(rng, left.n_sites - 1, right.n_sites - 1)
        code, info = pg.fb_route(left, right, band)
        tag = "seed %d tree %d (%d leaves x %d) node %d" % (seed0, tree, leaves, length, k)
        if code != 3:
            if info["widest"] > 1024:
                print(tag, "not eligible (widest diagonal %d)" % info["widest"], flush=True)
                continue
            bad += 1
            print("BAD", tag, "routes to schedule", code, info, flush=True)
            continue
        seen["pairs"] += 1; seen["far_pairs"] += info["far_cells"] > 0; seen["segments>1"] += info["segments"] > 1; seen["min_D"].add(info["min_D"])
        if route_only:
            print(tag, info, flush=True)
            continue
        fb = pg.FullProbability(left, right, mp, band)
        lf, lb, post, logf = oracle.fb(left, right, mp, band=band)
        ok = fb.schedule == 3
        ok = ok and abs(fb.log_fwd - lf) <= TOL * max(1, abs(lf)) and abs(fb.log_bwd - lb) <= TOL * max(1, abs(lb))
        ok = ok and close_logs(fb.log_forward(), logf) and np.allclose(fb.posterior(), post, rtol=1e-7, atol=1e-12)
        fb.close()
        if not ok:
            bad += 1
            print("BAD", tag, info, fb.log_fwd, lf, fb.log_bwd, lb, flush=True)
print("sweep_fb_deep: seed %d, %d trees, %d deep-ring pairs (%d with far cells, %d with several segments, smallest D seen %s): %d bad"
      % (seed0, n_trees, seen["pairs"], seen["far_pairs"], seen["segments>1"], sorted(seen["min_D"]), bad), flush=True)
sys.exit(1 if bad else 0)
