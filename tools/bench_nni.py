"""Measurement: tree search by nearest-neighbour interchange (csrc/dp_anc_nni.inc) on the shapes tools/bench_brlen.py uses -- the
walk over bench.make_inputs' sequences and tree, then the gains and the search over the walk's alignment -- and on the 600-leaf
caterpillar of random DNA rows (one evaluation: there is no tree to find in random rows).  A tool, not a test.

One process; per workload one warm-up call, then `repeats` timed calls (3 by default), one JSON line:
  * one pagan_anc_nni_gains evaluation on the walk's tree: the medians (and the spread, min .. max) of nni_ms and fold_ms beside
    up_ms + down_ms of the same call;
  * beside nni_ms what the entry points there were before would cost for the same answer: an up pass per rearranged tree,
    2 x candidates x the measured up_ms;
  * a full search from the UPGMA tree of the alignment (Msa.alignment_tree()): rounds, swaps, loglik start -> end, the stages' ms.
Reported, not asserted.  Results go to stdout and, appended, to profiles/nni_bench.jsonl.
    python tools/bench_nni.py [repeats] [workload ...]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import bench
from pagan2_msa_amd import host
import pycheck_anc as A

args = sys.argv[1:]
repeats = int(args[0]) if args and args[0].isdigit() else 3
names_given = [a for a in args if not a.isdigit()]
ALL = ["cfg4_32x100kb_dna_anchored", "cfg5_512x10kb_dna_anchored", "cfg3_64x500aa_protein_full", "codon_16x1500_anchored",
       "caterpillar_600x4096_dna"]
chosen = names_given or ALL
OUT = os.path.join(ROOT, "profiles", "nni_bench.jsonl")


def emit(record):
    line = json.dumps(record)
    print(line, flush=True)
    with open(OUT, "a") as f:
        f.write(line + "\n")


def spread(values):
    return {"median": float(np.median(values)), "min": float(min(values)), "max": float(max(values))}


def gains_record(label, call, extra):
    call()
    infos = [call()["info"] for _ in range(repeats)]
    i = infos[0]
    ms = {k: spread([x[k] for x in infos]) for k in ("up_ms", "down_ms", "nni_ms", "fold_ms", "total_ms")}
    out = {"workload": label, "what": "one evaluation", "columns": i["columns"], "states": i["states"], "chunks": i["chunks"],
           "device_bytes": i["device_bytes"], "candidates": i["candidates"], "ms": ms,
           "nni_over_up_plus_down": ms["nni_ms"]["median"] / (ms["up_ms"]["median"] + ms["down_ms"]["median"]),
           "one_up_pass_per_rearranged_tree_ms": 2 * i["candidates"] * ms["up_ms"]["median"], "repeats": repeats}
    out.update(extra)
    emit(out)


def search_record(label, call, extra):
    t0 = time.perf_counter()
    found = call()
    i = found["info"]
    out = {"workload": label, "what": "search from the alignment's UPGMA tree", "status": i["status"], "rounds": i["rounds"], "swaps": i["swaps"],
           "up_passes": i["up_passes"], "loglik_start": i["loglik_start"], "loglik_end": i["loglik_end"],
           "ms": {k: i[k] for k in ("up_ms", "down_ms", "nni_ms", "fold_ms", "total_ms")}, "wall_ms": (time.perf_counter() - t0) * 1e3}
    out.update(extra)
    emit(out)


for workload in chosen:
    if workload.startswith("caterpillar"):
        n, L = 600, 4096
        left, right, branch = A.caterpillar(n, 0.2)
        rows = A.random_rows(n, L, 1, 7, share=0.1)
        gains_record(workload, lambda: host.anc_nni_gains(left, right, branch, rows, 1, A.BASE_FREQ), {"n": n})
        continue
    cfg, leaves, length, branch, sub, indel, mean_len, anchors, alphabet = bench.WORKLOADS[workload]
    names, seqs, newick = bench.make_inputs(workload)
    data_type = 3 if alphabet == "CODON" else 2 if len(alphabet) == 20 else 1
    t0 = time.perf_counter()
    msa = host.Msa(names, seqs, newick, use_anchors=anchors, data_type=data_type).align()
    walk_s = time.perf_counter() - t0
    rows = msa.alignment()
    bf = host.dna_base_frequencies(seqs) if data_type == 1 else None
    left, right, branch = host.newick_arrays(list(names), msa.newick)
    gains_record(workload, lambda: host.anc_nni_gains(left, right, branch, rows, data_type, bf), {"n": msa.n, "walk_wall_s": walk_s})
    ul, ur, ub = host.newick_arrays(list(names), msa.alignment_tree())
    search_record(workload, lambda: host.anc_nni_search(ul, ur, ub, rows, data_type, bf), {"n": msa.n})
    msa.close()
