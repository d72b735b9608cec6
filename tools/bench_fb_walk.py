"""Measurement: the forward/backward pass as the tree walk uses it (dp_fb_post.inc, host_tree.cpp).  No oracle.

Runs on cfg4's tree by default (32 x 100 kb, anchored); one warm-up, then `repeats` timed repeats, one process, JSON lines:
 (i)  the leaf pairs and the internal pairs of the tree, each group through full_probability_batch, then site_marginals_batch over
      the handles and path_support along every pair's Viterbi path.  Device times (HIP events) of the sweeps and of the new
      kernels are kept apart; the marginal passes' rate is 2 x 48 B x cells / time (each pass reads F and B of every cell:
      24 B + 24 B), as GB/s and as a fraction of the 8 TB/s HBM peak.  "passes_over_sweeps" is the two marginal passes' time over
      the sweeps' (forward and backward run side by side: over the longer of the two, and over their sum).
 (ii) the walk with full_probability 0 / 1 / 2 and with sample_path, wall clock.
    python tools/bench_fb_walk.py [leaves] [length] [repeats]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import pagan2_msa_amd as pg
from pagan2_msa_amd import host, synth

leaves = int(sys.argv[1]) if len(sys.argv) > 1 else 32
length = int(sys.argv[2]) if len(sys.argv) > 2 else 100000
repeats = int(sys.argv[3]) if len(sys.argv) > 3 else 5
HBM_PEAK = 8.0e12

names, seqs, nwk = synth.evolve_balanced(leaves, length, branch=0.01, sub=0.008, indel_start=0.0008, mean_len=4.0, seed=20240807 + 4)
t0 = time.perf_counter()
msa = host.Msa(names, seqs, nwk, use_anchors=1).align()
print("walk: %.1f s, %d internal nodes" % (time.perf_counter() - t0, msa.n_internal), file=sys.stderr, flush=True)


def is_plain(g):
    n = g.n_sites
    return bool(np.all(np.diff(g.bwd_off)[1:] == 1) and np.array_equal(g.bwd_src[:n - 1], np.arange(n - 1)))


groups = {"leaf pairs": [], "internal pairs": []}
for k in range(msa.n_internal):
    left, right, _model, band = msa.node_job(k)
    scope = "leaf pairs" if is_plain(left) and is_plain(right) else "internal pairs"
    groups[scope].append((left, right, msa.node_model_prob(k), band, msa.node_result(k).cols))


def run_pairs(scope, items):
    pairs = [it[:4] for it in items]
    rows = []
    for rep in range(repeats + 1):
        t = time.perf_counter()
        fbs = pg.full_probability_batch(pairs)
        t_sweeps = time.perf_counter() - t
        cells = sum(fb.cells for fb in fbs)
        fwd_ms, bwd_ms = sum(fb.forward_ms for fb in fbs), sum(fb.backward_ms for fb in fbs)
        t = time.perf_counter()
        pg.site_marginals_batch(fbs)
        t_marg = time.perf_counter() - t
        row_ms, col_ms = sum(fb.post_ms()[1] for fb in fbs), sum(fb.post_ms()[2] for fb in fbs)
        t = time.perf_counter()
        n_cols = 0
        for fb, it in zip(fbs, items):
            n_cols += fb.path_support(it[4]).shape[0]
        t_sup = time.perf_counter() - t
        gather_ms = sum(fb.post_ms()[0] for fb in fbs)
        sched = [fb.schedule for fb in fbs]
        for fb in fbs:
            fb.close()
        if rep == 0:
            continue
        passes_s = (row_ms + col_ms) / 1e3
        rows.append({"sweeps_wall_s": round(t_sweeps, 4), "forward_ms": round(fwd_ms, 3), "backward_ms": round(bwd_ms, 3),
                     "row_pass_ms": round(row_ms, 3), "col_pass_ms": round(col_ms, 3), "marginals_wall_s": round(t_marg, 4),
                     "gather_ms": round(gather_ms, 3), "support_wall_s": round(t_sup, 4),
                     "marginals_GBps": round(2 * 48 * cells / passes_s / 1e9, 1) if passes_s > 0 else None,
                     "fraction_of_hbm_peak": round(2 * 48 * cells / passes_s / HBM_PEAK, 4) if passes_s > 0 else None,
                     "passes_over_sweeps": [round((row_ms + col_ms) / max(fwd_ms, bwd_ms), 5), round((row_ms + col_ms) / (fwd_ms + bwd_ms), 5)]})
    print(json.dumps({"scope": scope, "pairs": len(pairs), "cells": cells, "path_columns": n_cols, "schedules": sched, "repeats": rows,
                      "env": {k: v for k, v in os.environ.items() if k.startswith("PAGAN_FB_")}}), flush=True)


for scope, items in groups.items():
    if items:
        run_pairs(scope, items)
del groups
msa.close()

for label, opts in (("full_probability=0", {}), ("full_probability=1", {"full_probability": 1}), ("full_probability=2", {"full_probability": 2}),
                    ("sample_path=1", {"sample_path": 1, "sample_seed": 1})):
    secs, dev = [], None
    for rep in range(repeats + 1):
        t = time.perf_counter()
        w = host.Msa(names, seqs, nwk, use_anchors=1, **opts).align()
        dt = time.perf_counter() - t
        if opts:
            fbm = [w.node_fb(k) for k in range(w.n_internal)]
            dev = {"sweeps_ms": round(sum(x[2] for x in fbm), 2), "support_and_marginals_ms": round(sum(x[3] for x in fbm), 3)}
        w.close()
        if rep > 0:
            secs.append(dt)
    print(json.dumps({"scope": "walk", "options": label, "leaves": leaves, "length": length, "seconds": [round(s, 3) for s in secs],
                      "median_s": round(float(np.median(secs)), 3), "device_ms_last": dev}), flush=True)
