"""Measurement: the expected-counts pass (dp_fb_counts.inc) beside the same pairs' own sweeps and marginal passes.  No oracle,
no reference.

One process, one warm-up then `repeats` timed repeats, JSON lines:
 (i)  on one leaf pair of cfg4's tree inside its tunnel (32 x 100 kb, anchored) and on the tree's root pair: pg_fb_counts +
      pg_fb_counts_fold's device time (HIP events) with and without the emission table, beside the pair's forward and backward
      sweeps (pagan_fb_kernel_ms) and its two marginal passes (pagan_fb_post_ms) of the same repeat; bytes per cell = the pair's
      own F and B cells read once (48 B) over the pass's time as GB/s, and the ratio to the forward sweep.  Every repeat runs the
      pair's sweeps afresh.
 (ii) on cfg2's 15 node pairs (16 x 2 kb, full matrices) in ONE batch: the batch's counts launch beside the batch's sweeps and
      marginal launches.
    python tools/bench_fb_counts.py [repeats] [cfg4 leaves] [cfg4 length]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import pagan2_msa_amd as pg
from pagan2_msa_amd import host, synth

repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 5
leaves = int(sys.argv[2]) if len(sys.argv) > 2 else 32
length = int(sys.argv[3]) if len(sys.argv) > 3 else 100000


def is_plain(g):
    n = g.n_sites
    return bool(np.all(np.diff(g.bwd_off)[1:] == 1) and np.array_equal(g.bwd_src[:n - 1], np.arange(n - 1)))


def pairs_of(msa):
    out = []
    for k in range(msa.n_internal):
        left, right, _model, band = msa.node_job(k)
        out.append((left, right, msa.node_model_prob(k), band))
    return out


def measure(label, pairs):
    """the pairs as one batch: sweeps, marginal passes, counts with and without the table, per repeat"""
    rows = []
    cells = 0
    for rep in range(repeats + 1):
        fbs = pg.full_probability_batch(pairs)
        cells = sum(fb.cells for fb in fbs)
        fwd, bwd = sum(fb.forward_ms for fb in fbs), sum(fb.backward_ms for fb in fbs)
        t = time.perf_counter()
        with_table = pg.expected_counts_batch(fbs, True)
        wall = time.perf_counter() - t
        ms_table = sum(fb.counts_ms() for fb in fbs)
        pg.expected_counts_batch(fbs, False)
        ms_lean = sum(fb.counts_ms() for fb in fbs)
        pg.site_marginals_batch(fbs)
        rows_ms, cols_ms = sum(fb.post_ms()[1] for fb in fbs), sum(fb.post_ms()[2] for fb in fbs)
        ends = [float(c["end"].sum()) for c in with_table]
        for fb in fbs:
            fb.close()
        if rep > 0:
            rows.append({"counts_ms": round(ms_table, 4), "counts_no_table_ms": round(ms_lean, 4), "forward_ms": round(fwd, 4),
                         "backward_ms": round(bwd, 4), "marginal_rows_ms": round(rows_ms, 4), "marginal_columns_ms": round(cols_ms, 4),
                         "counts_over_forward": round(ms_table / fwd, 4) if fwd > 0 else None,
                         "own_cells_GB_per_s": round(48.0 * cells / (ms_table * 1e6), 2), "call_wall_s": round(wall, 5),
                         "end_counts_sum_min": round(min(ends), 9)})
    med = lambda key: round(float(np.median([r[key] for r in rows])), 4)
    print(json.dumps({"scope": label, "pairs": len(pairs), "cells": int(cells), "schedules": sorted({fb_s for fb_s in schedules(pairs)}),
                      "median": {k: med(k) for k in ("counts_ms", "counts_no_table_ms", "forward_ms", "backward_ms", "marginal_rows_ms",
                                                     "marginal_columns_ms", "counts_over_forward", "own_cells_GB_per_s")},
                      "repeats": rows}), flush=True)


def schedules(pairs):
    return [pg.fb_route(p[0], p[1], p[3])[0] for p in pairs]


t0 = time.perf_counter()
names, seqs, nwk = synth.evolve_balanced(leaves, length, branch=0.01, sub=0.008, indel_start=0.0008, mean_len=4.0, seed=20240807 + 4)
msa = host.Msa(names, seqs, nwk, use_anchors=1).align()
print("cfg4 walk: %.1f s, %d internal nodes" % (time.perf_counter() - t0, msa.n_internal), file=sys.stderr, flush=True)
all4 = pairs_of(msa)
leaf_k = next(k for k in range(msa.n_internal) if all(is_plain(g) for g in all4[k][:2]))
measure("cfg4 leaf pair (tunnel)", [all4[leaf_k]])
measure("cfg4 root pair (tunnel)", [all4[msa.n_internal - 1]])
del all4
msa.close()

names, seqs, nwk = synth.evolve_balanced(16, 2000, branch=0.05, sub=0.04, indel_start=0.004, mean_len=4.0, seed=20240807 + 2)
msa = host.Msa(names, seqs, nwk, use_anchors=0).align()
measure("cfg2 15 pairs, one batch (full matrices)", pairs_of(msa))
msa.close()
