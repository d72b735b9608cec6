"""Measurement: the guide tree from the sequences (csrc/dp_guide.hip, csrc/host_guide.cpp) on the sequence sets of cfg4
(32 x 100 kb) and cfg5 (512 x 10 kb), made by bench.make_inputs.  A tool, not a test.

One process; per workload one warm-up call, then `repeats` timed calls of host.guide_tree, JSON lines:
  * pack / sort / compress / pair-kernel device ms (HIP events, pagan_guide_info) and UPGMA host ms, medians; pairs per second;
  * the pair kernel's achieved bytes/s over its algorithmic bytes: 12 B per list entry, both lists read once per pair;
  * the same S from the numpy reading (np.unique lists, np.intersect1d) on one CPU thread: timed on `sample` pairs, checked
    against the device's integers, and scaled to all pairs;
  * the whole call's wall time as a share of the walk's recorded wall time for the workload (e2e_wall_s of BENCH_r06.json for
    cfg4 -- where that record has none, its ms_per_step, the device-resident pass, which is less than the walk: the share is
    then an upper bound -- and of profiles/r05_bench_cfg5_one_gpu.json for cfg5).
    python tools/bench_guide_tree.py [repeats] [sample]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ.setdefault("OMP_NUM_THREADS", "1")
import numpy as np
import bench
from pagan2_msa_amd import host
import pycheck_guide as G

repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 5
sample = int(sys.argv[2]) if len(sys.argv) > 2 else 200


def recorded_walk_s(workload):
    if workload.startswith("cfg4"):
        with open(os.path.join(ROOT, "BENCH_r06.json")) as f:
            p = json.load(f)["parsed"]
        if p.get("e2e_wall_s"):
            return p["e2e_wall_s"], "BENCH_r06.json e2e_wall_s"
        return p["ms_per_step"] / 1e3, "BENCH_r06.json ms_per_step (no e2e_wall_s recorded: the share is an upper bound)"
    with open(os.path.join(ROOT, "profiles", "r05_bench_cfg5_one_gpu.json")) as f:
        return json.load(f)["e2e_wall_s"], "profiles/r05_bench_cfg5_one_gpu.json e2e_wall_s"


def timed(names, seqs):
    host.guide_tree(names, seqs)
    infos, walls = [], []
    for _ in range(repeats):
        t0 = time.perf_counter()
        _, info = host.guide_tree(names, seqs, with_info=True)
        walls.append(time.perf_counter() - t0)
        infos.append(info)
    med = {k: float(np.median([i[k] for i in infos])) for k in ("pack_ms", "sort_ms", "compress_ms", "pairs_ms", "upgma_ms")}
    return infos[0], med, float(np.median(walls))


for workload in ("cfg4_32x100kb_dna_anchored", "cfg5_512x10kb_dna_anchored"):
    names, seqs, _ = bench.make_inputs(workload)
    n = len(seqs)
    info, med, wall = timed(names, seqs)
    k = info["k"]
    # the lists as numpy has them: entries per sequence -> the pair kernel's algorithmic bytes
    t0 = time.perf_counter()
    lists = [np.unique(G.packed_codes(s, k, 1), return_counts=True) for s in seqs]
    lists_s = time.perf_counter() - t0
    entries = np.array([len(c) for c, _ in lists], np.int64)
    assert int(entries.sum()) == info["entries"]
    alg_bytes = 12 * int(entries.sum()) * (n - 1)                      # every list is read once for each of its n - 1 pairs
    shared, _, _, _ = host.guide_distances(seqs)
    rng = np.random.default_rng(0)
    t0 = time.perf_counter()
    for _ in range(sample):
        x, y = sorted(rng.choice(n, 2, replace=False))
        (ca, na), (cb, nb) = lists[x], lists[y]
        _, ia, ib = np.intersect1d(ca, cb, assume_unique=True, return_indices=True)
        assert int(np.minimum(na[ia], nb[ib]).sum()) == shared[x, y]
    numpy_pairs_s = (time.perf_counter() - t0) / sample * info["pairs"]
    walk_s, walk_src = recorded_walk_s(workload)
    out = {"workload": workload, "n": n, "k": k, "positions": info["positions"], "entries": info["entries"], "pairs": info["pairs"],
           "waves_per_pair": info["waves_per_pair"], "device_bytes": info["device_bytes"], "median_ms": med,
           "pairs_per_s": info["pairs"] / (med["pairs_ms"] / 1e3), "pair_kernel_algorithmic_bytes": alg_bytes,
           "pair_kernel_GBps": alg_bytes / (med["pairs_ms"] / 1e3) / 1e9, "guide_tree_wall_s": wall,
           "numpy_one_thread_s": {"lists": lists_s, "pairs_scaled_from_sample": numpy_pairs_s, "sample": sample},
           "walk_s": walk_s, "walk_source": walk_src, "share_of_walk": wall / walk_s, "repeats": repeats}
    print(json.dumps(out), flush=True)
