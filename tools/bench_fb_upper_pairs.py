"""Measurement: forward/backward over the internal-node pairs ABOVE the leaves of a guide tree (graph pairs inside their tunnels),
the workload the deep-ring sweeps (dp_fb_deep.inc) exist for.  No oracle.

Walks the tree once on the GPU (cfg4 by default: 32 x 100 kb, anchored), takes every pair above the leaves with msa.node_job,
and times pagan_fb_run_batch (wall clock around the call: staging, launches, synchronisation) on all of them at once and level by
level: one warm-up, then `repeats` timed calls, one process.  Prints one JSON line per repeat set ("scope": "all" or "level N")
with cells/s of every repeat (cells over the wall clock of a pass of both sweeps, as bench.py counts), and -- where the library has pagan_fb_debug_route -- the routing and the plan's figures per pair.
The same script runs on a commit without the deep ring (it then reports schedules from pagan_fb_groups only), which is how the
two are compared:
    python tools/bench_fb_upper_pairs.py [leaves] [length] [repeats]
    PAGAN_FB_DEEP=0 python tools/bench_fb_upper_pairs.py            # the new code on the old route"""
import ctypes as C
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

names, seqs, nwk = synth.evolve_balanced(leaves, length, branch=0.01, sub=0.008, indel_start=0.0008, mean_len=4.0, seed=20240807 + 4)
t0 = time.perf_counter()
msa = host.Msa(names, seqs, nwk, use_anchors=1).align()
print("walk: %.1f s, %d internal nodes" % (time.perf_counter() - t0, msa.n_internal), file=sys.stderr, flush=True)
bf = np.array([sum(s.count(x) for s in seqs) for x in "ACGT"], np.float32)
bf /= bf.sum()


def is_plain(g):
    n = g.n_sites
    return bool(np.all(np.diff(g.bwd_off)[1:] == 1) and np.array_equal(g.bwd_src[:n - 1], np.arange(n - 1)))


def reaches(g):
    off = g.bwd_off.astype(np.int64)
    idx = np.repeat(np.arange(g.n_sites), np.diff(off))
    keep = (idx >= 1) & (idx < g.n_sites - 1)
    r = np.zeros(g.n_sites, np.int64)
    np.maximum.at(r, idx[keep], idx[keep] - g.bwd_src[:off[-1]][keep])
    return r


pairs, levels, cells = [], [], []
for k in range(msa.n_internal):
    left, right, _model, band = msa.node_job(k)
    if is_plain(left) and is_plain(right):
        continue
    pairs.append((left, right, host.model_prob(1, msa.node_info(k).dist, base_freq=bf), band))
    levels.append(int(msa.node_info(k).level))
    cells.append(int(pg.lib().pagan_dp_count_cells(left.n_sites, right.n_sites, C.byref(band.c) if band is not None else None)))
    row = {"node": k, "level": levels[-1], "sites": [left.n_sites - 1, right.n_sites - 1], "cells": cells[-1],
           "multi_edge_sites": [int((np.diff(left.bwd_off) > 1).sum()), int((np.diff(right.bwd_off) > 1).sum())]}
    rl, rr = reaches(left), reaches(right)
    row["sites_with_reach_ge"] = {str(t): [int((rl >= t).sum()), int((rr >= t).sum())] for t in (4, 8, 16, 32, 64)}
    if hasattr(pg, "fb_route"):
        code, info = pg.fb_route(left, right, band)
        row["route"] = code
        row.update(info)
        row["far_cell_share"] = info["far_cells"] / max(cells[-1], 1)
        row["far_diagonal_share"] = info["far_diagonals"] / max(info["diagonals"], 1)
    print(json.dumps({"pair": row}), flush=True)


def run(scope, idx):
    sub = [pairs[q] for q in idx]
    n_cells = sum(cells[q] for q in idx)
    n_diag = max(p[0].n_sites + p[1].n_sites - 3 for p in sub)
    secs, sched = [], None
    for rep in range(repeats + 1):
        t = time.perf_counter()
        fbs = pg.full_probability_batch(sub)
        dt = time.perf_counter() - t
        sched = [getattr(fb, "schedule", 1 if fb.groups > 1 else (2 if fb.groups == 0 else 0)) for fb in fbs]
        kms = [sum(fb.forward_ms for fb in fbs), sum(fb.backward_ms for fb in fbs)]
        for fb in fbs:
            fb.close()
        if rep > 0:
            secs.append(dt)
    print(json.dumps({"scope": scope, "pairs": len(sub), "cells": n_cells, "schedules": sched, "seconds": [round(s, 4) for s in secs],
                      "cells_per_s": [round(n_cells / s) for s in secs],            # (bench.py's convention: cells over the time of a pass of both sweeps)
                      "slowest_cells_per_s": round(n_cells / max(secs)), "median_cells_per_s": round(n_cells / float(np.median(secs))),
                      "fastest_cells_per_s": round(n_cells / min(secs)),
                      "kernel_ms_last": [round(x, 2) for x in kms], "us_per_diagonal_of_the_longest_pair": round(1e6 * min(secs) / n_diag, 3),
                      "env": {k: v for k, v in os.environ.items() if k.startswith("PAGAN_FB_")}}), flush=True)


run("all", list(range(len(pairs))))
for lv in sorted(set(levels)):
    run("level %d" % lv, [q for q in range(len(pairs)) if levels[q] == lv])
