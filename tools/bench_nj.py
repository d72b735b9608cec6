"""Measurement: neighbour joining on the device (csrc/dp_nj.hip, csrc/host_nj.cpp) on cfg5's k-mer distances (n = 512,
bench.make_inputs and host.guide_distances) and on synthetic matrices of n = 2,048 and 4,096: the leaf distances of a random
tree without a clock, every entry times 1 + 5 % noise.  A tool, not a test.

One process; per matrix one warm-up call, then `repeats` timed calls of host.nj_tree (5 by default), one JSON line:
  * scan / pick / merge device ms (PAGAN_NJ_EVENTS=1: HIP events between the launches, pagan_nj_info), their sum per join in us,
    and loop_ms (two events) of those calls;
  * the scan's bytes -- 8 per matrix entry it reads, summed over the joins (pagan_nj_info.scan_entries) -- over scan_ms;
  * the rooting's host ms, and the call as it runs by default, without the events between the launches: loop_ms, us per join
    and the wall time (wall_ms is the measured call's, events included);
  * host.guide_upgma's wall time on the same matrix, for scale.
With `refine`: align_refined(rounds=2) on the two families tools/bench_brlen.py uses (DNA 16 x 2 kb, protein 16 x 300 aa), UPGMA
against NJ, each with and without branch_lengths="ml": columns, score, log likelihood and the clades of the last walk's tree the
simulated tree does not have.  Reported, not asserted.  Results go to stdout and, appended, to profiles/nj_bench.jsonl.
    python tools/bench_nj.py [--repeats R] [512 | 2048 | 4096 | refine ...]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import bench
from pagan2_msa_amd import host, synth
import pycheck_anc as A

args = sys.argv[1:]
repeats = 5
if "--repeats" in args:
    at = args.index("--repeats")
    repeats = int(args[at + 1])
    del args[at:at + 2]
chosen = args or ["512", "2048", "4096", "refine"]
OUT = os.path.join(ROOT, "profiles", "nj_bench.jsonl")


def emit(record):
    line = json.dumps(record)
    print(line, flush=True)
    with open(OUT, "a") as f:
        f.write(line + "\n")


def noisy_tree_matrix(n, seed, noise=0.05):
    """Leaf distances of a random binary tree built by joining random clusters under branches of 0.01 .. 0.2 (no clock), then
    every entry times 1 + noise * uniform(-1, 1), symmetric."""
    rng = np.random.default_rng(seed)
    d = np.zeros((n, n))
    depth = np.zeros(n)
    groups = [np.array([k]) for k in range(n)]
    while len(groups) > 1:
        i, j = sorted(rng.choice(len(groups), 2, replace=False))
        a, b = groups[i], groups[j]
        la, lb = rng.uniform(0.01, 0.2, 2)
        across = (depth[a] + la)[:, None] + (depth[b] + lb)[None, :]
        d[np.ix_(a, b)] = across
        d[np.ix_(b, a)] = across.T
        depth[a] += la
        depth[b] += lb
        groups[i] = np.concatenate([a, b])
        groups.pop(j)
    d *= 1 + noise * np.triu(rng.uniform(-1, 1, (n, n)), 1)
    return np.triu(d, 1) + np.triu(d, 1).T


def timed(names, dist, events):
    if events:
        os.environ["PAGAN_NJ_EVENTS"] = "1"
    else:
        os.environ.pop("PAGAN_NJ_EVENTS", None)
    host.nj_tree(names, dist)
    infos, walls = [], []
    for _ in range(repeats):
        t0 = time.perf_counter()
        _, info = host.nj_tree(names, dist, with_info=True)
        walls.append((time.perf_counter() - t0) * 1e3)
        infos.append(info)
    os.environ.pop("PAGAN_NJ_EVENTS", None)
    med = {k: float(np.median([i[k] for i in infos])) for k in ("scan_ms", "pick_ms", "merge_ms", "loop_ms", "root_ms")}
    return infos[0], med, float(np.median(walls))


def measure(label, dist):
    n = len(dist)
    names = ["s%d" % k for k in range(n)]
    info, med, wall = timed(names, dist, True)
    _, bare, bare_wall = timed(names, dist, False)
    host.guide_upgma(names, dist)
    upgma = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        host.guide_upgma(names, dist)
        upgma.append((time.perf_counter() - t0) * 1e3)
    stages = med["scan_ms"] + med["pick_ms"] + med["merge_ms"]
    emit({"matrix": label, "n": n, "joins": info["joins"], "launches": info["launches"], "device_bytes": info["device_bytes"],
          "median_ms": med, "us_per_join": stages / info["joins"] * 1e3, "scan_bytes": 8 * info["scan_entries"],
          "scan_GBps": 8 * info["scan_entries"] / (med["scan_ms"] / 1e3) / 1e9, "wall_ms": wall,
          "default_call": {"loop_ms": bare["loop_ms"], "us_per_join": bare["loop_ms"] / info["joins"] * 1e3, "wall_ms": bare_wall},
          "upgma_host_ms": float(np.median(upgma)), "repeats": repeats})


def refine():
    families = {"dna_16x2kb": (synth.evolve_balanced(16, 2000, branch=0.05, sub=0.05, indel_start=0.005, mean_len=3, seed=31), {"use_anchors": 1}),
                "protein_16x300aa": (synth.evolve_balanced(16, 300, branch=0.08, sub=0.08, indel_start=0.01, mean_len=2, seed=32, alphabet=A.PROTEIN),
                                     {"use_anchors": 0, "data_type": 2})}
    for label, ((names, seqs, truth), opts) in families.items():
        for method in ("upgma", "nj"):
            for mode in (None, "ml"):
                t0 = time.perf_counter()
                msa = host.align_refined(names, seqs, rounds=2, branch_lengths=mode, tree_method=method, **opts)
                last = msa.history[-1]
                emit({"refine": label, "tree_method": method, "branch_lengths": mode, "walks": len(msa.history),
                      "columns": last["alignment_length"], "score": last["score"], "loglik": msa.ancestral().loglik,
                      "clades_not_in_simulated_tree": host.differing_clades(msa.newick, truth),
                      "first_tree_clades_not_in_simulated_tree": host.differing_clades(msa.history[0]["newick"], truth),
                      "wall_s": time.perf_counter() - t0})
                msa.close()


for what in chosen:
    if what == "refine":
        refine()
    elif what == "512":
        _, seqs, _ = bench.make_inputs("cfg5_512x10kb_dna_anchored")
        measure("cfg5_512x10kb k-mer distances", host.guide_distances(seqs)[2])
    else:
        measure("tree + 5 %% noise, n = %s" % what, noisy_tree_matrix(int(what), int(what)))
