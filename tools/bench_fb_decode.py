"""Measurement: posterior decoding on the device (dp_fb_decode.inc) beside the existing code it sits next to.  No oracle.

Runs on cfg4's tree by default (32 x 100 kb, anchored); one warm-up, then `repeats` timed repeats, one process, JSON lines:
 (i)  on one leaf pair of the tree inside its tunnel (decode route 1: pg_fb_ring_decode) and on the tree's root pair (route 0:
      pg_fb_decode_fill): the decode fill's and the trace's device time (HIP events), the fill's us per cell diagonal, the wall
      clock of the call; beside them, in the same repeat, the same pair's forward sweep (pagan_fb_kernel_ms) and a K = 1
      sample_paths call.  "condition_ring" (leaf pair only): the decode fill takes no longer than the pair's forward ring sweep
      of the same repeat, no margin.  Every repeat runs the pair's sweeps afresh.
 (ii) the walk with full_probability=1, with sample_path=1 (sampler on the device) and with posterior_decode=1, wall clock.
    python tools/bench_fb_decode.py [leaves] [length] [repeats]"""
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
GAP_WEIGHT = 0.5
SEED = 1

names, seqs, nwk = synth.evolve_balanced(leaves, length, branch=0.01, sub=0.008, indel_start=0.0008, mean_len=4.0, seed=20240807 + 4)
t0 = time.perf_counter()
msa = host.Msa(names, seqs, nwk, use_anchors=1).align()
print("walk: %.1f s, %d internal nodes" % (time.perf_counter() - t0, msa.n_internal), file=sys.stderr, flush=True)


def is_plain(g):
    n = g.n_sites
    return bool(np.all(np.diff(g.bwd_off)[1:] == 1) and np.array_equal(g.bwd_src[:n - 1], np.arange(n - 1)))


def pair_of(k):
    left, right, _model, band = msa.node_job(k)
    return left, right, msa.node_model_prob(k), band


leaf_k = next(k for k in range(msa.n_internal) if all(is_plain(g) for g in msa.node_job(k)[:2]))
scopes = (("leaf pair", leaf_k), ("root pair", msa.n_internal - 1))


def run_pair(scope, k):
    left, right, mp, band = pair_of(k)
    node = leaves + k
    nd = left.n_sites + right.n_sites - 3
    route = pg.fb_decode_route(left, right, band)
    rows = []
    cells = 0
    for rep in range(repeats + 1):
        fb = pg.FullProbability(left, right, mp, band)
        cells = fb.cells
        t = time.perf_counter()
        dec = fb.decode(GAP_WEIGHT)
        t_call = time.perf_counter() - t
        sm = dec.summary()
        assert sm["status"] == 0 and sm["schedule"] == route
        fill_ms, trace_ms = dec.ms()
        dec.close()
        t = time.perf_counter()
        sp = fb.sample_paths(SEED, node, 1)
        t_sample = time.perf_counter() - t
        row = {"decode": {"fill_ms": round(fill_ms, 3), "trace_ms": round(trace_ms, 3), "fill_us_per_diagonal": round(1e3 * fill_ms / nd, 4),
                          "call_wall_s": round(t_call, 5), "steps": sm["n_steps"], "objective": sm["objective"]},
               "forward_sweep": {"schedule": fb.schedule, "ms": round(fb.forward_ms, 3), "us_per_diagonal": round(1e3 * fb.forward_ms / nd, 4)},
               "sample_K1": {"kernel_ms": round(sp.ms, 3), "call_wall_s": round(t_sample, 5)}}
        if route == 1:
            row["condition_ring"] = {"decode_fill_ms": round(fill_ms, 3), "forward_ring_ms": round(fb.forward_ms, 3),
                                     "forward_is_ring": fb.schedule == 2, "met": bool(fb.schedule == 2 and fill_ms <= fb.forward_ms)}
        sp.close()
        fb.close()
        if rep > 0:
            rows.append(row)
    print(json.dumps({"scope": scope, "node": k, "sites": [left.n_sites, right.n_sites], "cells": int(cells), "diagonals": nd,
                      "banded": band is not None, "decode_route": route, "gap_weight": GAP_WEIGHT, "repeats": rows}), flush=True)


for scope, k in scopes:
    run_pair(scope, k)
msa.close()

for label, opts in (("full_probability=1", {"full_probability": 1}),
                    ("sample_path=1, sampler on the device", {"sample_path": 1, "sample_seed": SEED, "sample_on_device": 1}),
                    ("posterior_decode=1", {"posterior_decode": 1, "decode_gap_weight": GAP_WEIGHT})):
    secs, dev = [], None
    for rep in range(repeats + 1):
        t = time.perf_counter()
        w = host.Msa(names, seqs, nwk, use_anchors=1, **opts).align()
        dt = time.perf_counter() - t
        fbm = [w.node_fb(k) for k in range(w.n_internal)]
        dev = {"sweeps_ms": round(sum(x[2] for x in fbm), 2), "support_and_sampler_ms": round(sum(x[3] for x in fbm), 3)}
        if "posterior_decode" in opts:
            dev["decode_ms"] = round(sum(w.node_decode(k)[2] for k in range(w.n_internal)), 3)
        w.close()
        if rep > 0:
            secs.append(dt)
    print(json.dumps({"scope": "walk", "options": label, "leaves": leaves, "length": length,
                      "seconds": [round(s, 3) for s in secs], "median_s": round(float(np.median(secs)), 3), "device_ms_last": dev}), flush=True)
