"""Measurement: path sampling on the device (dp_fb_sample.inc, pg_fb_sample) beside the host sampler it restates.  No oracle.

Runs on cfg4's tree by default (32 x 100 kb, anchored); one warm-up, then `repeats` timed repeats, one process, JSON lines:
 (i)  on one leaf pair of the tree inside its tunnel and on the tree's root pair, K = 1, 64, 1024 paths drawn on the device: the
      kernel's device time (HIP events), the wall clock of the call around it (upload of the records, launch, summaries back)
      and, apart, the wall clock of downloading ALL K traces in one copy (visited_all).  Beside it the same paths through
      pagan_fb_sample_path: the first call's matrix download + walk, then K - 1 more walks, wall clock (the uniform numbers'
      generation included on both sides: the device computes its own).  The host's K = 1024 is timed at 64 walks and scaled, and
      says so.  "condition_K64": device call + download of all 64 traces <= the host's download + 64 walks, per repeat.
      Every repeat runs the pair's sweeps afresh (the host sampler caches the downloaded matrix in the handle).
 (ii) the walk with sample_path=1, sampler on the host and on the device, wall clock.
    python tools/bench_fb_sample.py [leaves] [length] [repeats]"""
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
KS = (1, 64, 1024)
HOST_WALKS = 64
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
    n_u = left.n_sites + right.n_sites - 1
    rows = []
    cells = 0
    for rep in range(repeats + 1):
        fb = pg.FullProbability(left, right, mp, band)
        cells = fb.cells
        row = {"device": {}, "host": {}}
        for K in KS:
            t = time.perf_counter()
            sp = fb.sample_paths(SEED, node, K)
            t_call = time.perf_counter() - t
            t = time.perf_counter()
            _vis, n = sp.visited_all()
            t_down = time.perf_counter() - t
            sm = sp.summary()
            assert not sm["status"].any()
            row["device"][str(K)] = {"kernel_ms": round(sp.ms, 3), "call_wall_s": round(t_call, 5), "traces_download_wall_s": round(t_down, 5),
                                     "trace_bytes": int(12 * K * (n_u - 1)), "steps_mean": round(float(n.mean()), 1), "steps_max": int(n.max())}
            del _vis
            sp.close()
        t = time.perf_counter()
        fb.sample_path(host.sample_uniforms_path(SEED, node, 0, n_u))
        t_first = time.perf_counter() - t
        t = time.perf_counter()
        for p in range(1, HOST_WALKS):
            fb.sample_path(host.sample_uniforms_path(SEED, node, p, n_u))
        t_rest = time.perf_counter() - t
        per_walk = t_rest / (HOST_WALKS - 1)
        row["host"] = {"download_and_first_walk_s": round(t_first, 5), "walk_s": round(per_walk, 5), "matrix_bytes": int(24 * cells),
                       "1": round(t_first, 5), "64": round(t_first + t_rest, 5), "1024": round(t_first + 1023 * per_walk, 4),
                       "1024_is_scaled_from_walks": HOST_WALKS}
        d64 = row["device"]["64"]
        row["condition_K64"] = {"device_s": round(d64["call_wall_s"] + d64["traces_download_wall_s"], 5), "host_s": row["host"]["64"],
                                "met": bool(d64["call_wall_s"] + d64["traces_download_wall_s"] <= t_first + t_rest)}
        fb.close()
        if rep > 0:
            rows.append(row)
    print(json.dumps({"scope": scope, "node": k, "sites": [left.n_sites, right.n_sites], "cells": int(cells), "banded": band is not None,
                      "repeats": rows}), flush=True)


for scope, k in scopes:
    run_pair(scope, k)
msa.close()

for label, on_device in (("sampler on the host", 0), ("sampler on the device", 1)):
    secs, dev = [], None
    for rep in range(repeats + 1):
        t = time.perf_counter()
        w = host.Msa(names, seqs, nwk, use_anchors=1, sample_path=1, sample_seed=SEED, sample_on_device=on_device).align()
        dt = time.perf_counter() - t
        fbm = [w.node_fb(k) for k in range(w.n_internal)]
        dev = {"sweeps_ms": round(sum(x[2] for x in fbm), 2), "support_and_sampler_ms": round(sum(x[3] for x in fbm), 3)}
        w.close()
        if rep > 0:
            secs.append(dt)
    print(json.dumps({"scope": "walk", "options": "sample_path=1, " + label, "leaves": leaves, "length": length,
                      "seconds": [round(s, 3) for s in secs], "median_s": round(float(np.median(secs)), 3), "device_ms_last": dev}), flush=True)
